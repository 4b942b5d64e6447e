// The kernels of the obstacle focus (omds.h: omds_focus_obstacles; the host stage: obstacle_focus.hip).  The distances are pass 1's
// (mlp_kernels.hip); here are the keys of the reaches (obstacle_focus_def.h) and the selection: ONE workgroup of 1024 lanes runs an
// exact k-th-smallest twice on the keys -- a radix select, most significant byte first, over a 256-bin histogram in LDS -- once for the
// threshold of the n_closest-th sphere, once for the last kept sphere, and names the index at which the group of keys equal to that
// last one is cut.  The ordered compaction of cloud_kernels.hip (FocusSrc) then emits the kept spheres in ascending index.
// The keys stay in global memory (256 KB at 65 536 spheres: L2) and every pass strides over them, so one code path takes any count.
// Integer arithmetic throughout: the LDS atomics are integer adds, whose sum no order changes, and nothing reads a value an atomic
// returns; the result is a function of the keys alone.
// A focus along a PATH of states (omds_focus_obstacles_path) takes the states in chunks of C: the keys of the chunk's C x n reaches
// in place over pass 1's rows, per row the bar of its own n_closest-th key (C workgroups, the same k-th-smallest), and the merge of
// "passes in some row" and "the nearest key" into two words per sphere that live across the chunks -- integer OR and minimum, global
// atomics nothing reads back, so neither the chunking nor the scheduling shows.  The words of the passing spheres (the others: a
// word above every key) then go through the same selection and the same compaction.
#include "cloud_kernels.h"
#include "obstacle_focus_def.h"

namespace {

constexpr int FOCUS_NT = 1024, FOCUS_WAVES = FOCUS_NT / 64;

// keys [n] of the reaches: vel == nullptr -> the distance itself; dims < 3 (a planar-point network) -> v_z = 0, as the horizon moves
// such a scene
__global__ __launch_bounds__(CLOUD_NT) void k_focus_keys(const float* __restrict__ d, const float* __restrict__ vel, int dims, float lookahead, int n,
                                                         unsigned* __restrict__ keys) {
    const int o = blockIdx.x * CLOUD_NT + threadIdx.x;
    if (o >= n) return;
    float r = d[o];
    if (vel) r = focus_reach(r, vel[3 * (size_t)o], vel[3 * (size_t)o + 1], dims < 3 ? 0.f : vel[3 * (size_t)o + 2], lookahead);
    keys[o] = focus_key(r);
}

struct FocusLds {
    unsigned hist[256];
    unsigned wsum[FOCUS_WAVES];
    unsigned pick[3];   // the digit chosen in a pass, the rank left inside its bin, the keys below the bin
    unsigned count;
};

__device__ inline unsigned wave_inclusive_scan(unsigned v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// The key of rank k (1 <= k <= n, ties counted) among keys [n]; *less = the keys strictly below it.  Four passes of eight bits: the
// keys that share the digits chosen so far are counted per next digit, and the first wave walks the 256 counts to the bin that holds
// rank k.  A lane adds a run of equal digits with one atomic: where a byte is the same for nearly every key (sign and exponent of
// distances of one magnitude) that is one add per lane and not one per key on a single LDS word.
__device__ unsigned focus_kth(const unsigned* __restrict__ keys, int n, unsigned k, FocusLds& s, unsigned* less) {
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned prefix = 0, mask = 0, below = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) s.hist[tid] = 0;
        __syncthreads();
        unsigned cur = 0, run = 0;
        for (int i = tid; i < n; i += FOCUS_NT) {
            const unsigned key = keys[i];
            if ((key & mask) != prefix) continue;
            const unsigned digit = key >> shift & 255u;
            if (digit != cur && run) {
                atomicAdd(&s.hist[cur], run);
                run = 0;
            }
            cur = digit;
            ++run;
        }
        if (run) atomicAdd(&s.hist[cur], run);
        __syncthreads();
        if (tid < 64) {   // lane l owns bins 4 l .. 4 l + 3
            const unsigned h[4] = {s.hist[4 * tid], s.hist[4 * tid + 1], s.hist[4 * tid + 2], s.hist[4 * tid + 3]};
            const unsigned sum = h[0] + h[1] + h[2] + h[3];
            const unsigned inc = wave_inclusive_scan(sum, lane);
            unsigned before = inc - sum;
            if (before < k && k <= inc) {   // exactly one lane: the counts of this pass add up to at least k
                int b = 0;
                while (before + h[b] < k) before += h[b++];
                s.pick[0] = (unsigned)(4 * tid + b);
                s.pick[1] = k - before;
                s.pick[2] = before;
            }
        }
        __syncthreads();
        prefix |= s.pick[0] << shift;
        mask |= 255u << shift;
        k = s.pick[1];
        below += s.pick[2];
    }
    *less = below;
    return prefix;
}

// sum of v over the workgroup, the same value in every lane
__device__ unsigned focus_block_sum(unsigned v, FocusLds& s) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();   // wsum may still be read from an earlier call
    if (lane == 0) s.wsum[w] = v;
    __syncthreads();
    unsigned t = 0;
    for (int i = 0; i < FOCUS_WAVES; ++i) t += s.wsum[i];
    return t;
}

// res[0] = M kept, res[1] = P passing, res[2] = the key of the last kept sphere of the order, res[3] = the index up to which (inclusive)
// a sphere with exactly that key is kept
// PATH: keys are the words k_focus_path_words left, and the passing spheres are those whose word is a key
template <bool PATH>
__global__ __launch_bounds__(FOCUS_NT) void k_focus_select(const unsigned* __restrict__ keys, int n, int n_closest, float margin, int all_pass,
                                                           int max_keep, unsigned* __restrict__ res) {
    __shared__ FocusLds s;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned passed = (unsigned)n, less;
    if (PATH) {
        unsigned c = 0;
        for (int i = tid; i < n; i += FOCUS_NT) c += keys[i] != FOCUS_NOT_PASSING;
        passed = focus_block_sum(c, s);
    } else if (!all_pass) {
        const unsigned bar = focus_bar_key(focus_kth(keys, n, (unsigned)n_closest, s, &less), margin);
        unsigned c = 0;
        for (int i = tid; i < n; i += FOCUS_NT) c += keys[i] <= bar;
        passed = focus_block_sum(c, s);
    }
    const unsigned kept = max_keep > 0 ? min(passed, (unsigned)max_keep) : passed;
    const unsigned last = focus_kth(keys, n, kept, s, &less);
    const unsigned take = kept - less;   // >= 1: of the keys equal to `last`, the first `take` in index order are kept
    // the index of the take-th of them: every lane counts those of its own contiguous range, the workgroup scans the counts in lane
    // order, and the one lane whose range holds it walks there
    const int per = (n + FOCUS_NT - 1) / FOCUS_NT;
    const int lo = (int)min((long long)tid * per, (long long)n), hi = (int)min((long long)lo + per, (long long)n);
    unsigned mine = 0;
    for (int i = lo; i < hi; ++i) mine += keys[i] == last;
    const unsigned inc = wave_inclusive_scan(mine, lane);
    __syncthreads();
    if (lane == 63) s.wsum[w] = inc;
    __syncthreads();
    unsigned before = inc - mine;
    for (int i = 0; i < w; ++i) before += s.wsum[i];
    if (before < take && take <= before + mine) {
        int i = lo;
        for (unsigned seen = before;; ++i)
            if (keys[i] == last && ++seen == take) break;
        res[0] = kept;
        res[1] = passed;
        res[2] = last;
        res[3] = (unsigned)i;
    }
}

// ---- a focus along a path: one chunk of C states, rows [C][n] (row b at rows + b n) --------------------------------------------------

constexpr int PATH_ROWS = 16;   // rows of a chunk one workgroup of the keys and of the merge walks

// the keys of the chunk's reaches, in place over pass 1's distances; time [C]: lookahead + ahead of every state (vel given), the speed
// of a sphere computed once per lane
__global__ __launch_bounds__(CLOUD_NT) void k_focus_path_keys(unsigned* __restrict__ rows, const float* __restrict__ vel, int dims,
                                                              const float* __restrict__ time, int C, int n) {
    const int o = blockIdx.x * CLOUD_NT + threadIdx.x;
    if (o >= n) return;
    const int b0 = blockIdx.y * PATH_ROWS, b1 = min(b0 + PATH_ROWS, C);
    float speed = 0.f;
    if (vel) speed = focus_speed(vel[3 * (size_t)o], vel[3 * (size_t)o + 1], dims < 3 ? 0.f : vel[3 * (size_t)o + 2]);
    for (int b = b0; b < b1; ++b) {
        unsigned* p = rows + (size_t)b * n + o;
        float r = focus_float(*p);
        if (vel) r = fmaf(-speed, time[b], r);
        *p = focus_key(r);
    }
}

// bars [C]: workgroup b holds the bar of row b
__global__ __launch_bounds__(FOCUS_NT) void k_focus_path_bars(const unsigned* __restrict__ rows, int n, int n_closest, float margin,
                                                              unsigned* __restrict__ bars) {
    __shared__ FocusLds s;
    unsigned less;
    const unsigned kth = focus_kth(rows + (size_t)blockIdx.x * n, n, (unsigned)n_closest, s, &less);
    if (threadIdx.x == 0) bars[blockIdx.x] = focus_bar_key(kth, margin);
}

// A lane owns V consecutive spheres (V = 4: n is a multiple of 4 and every row starts at a multiple of 16 bytes) and walks PATH_ROWS
// rows of the chunk; what it found goes into best [n] (minimum) and pass [n] (OR), which the caller set to ~0 and 0 before the
// first chunk
template <int V>
__global__ __launch_bounds__(CLOUD_NT) void k_focus_path_merge(const unsigned* __restrict__ rows, const unsigned* __restrict__ bars, int all_pass,
                                                               int C, int n, unsigned* __restrict__ best, unsigned* __restrict__ pass) {
    __shared__ unsigned bar[PATH_ROWS];
    const int b0 = blockIdx.y * PATH_ROWS, nb = min(PATH_ROWS, C - b0);
    if ((int)threadIdx.x < nb) bar[threadIdx.x] = all_pass ? FOCUS_NOT_PASSING : bars[b0 + threadIdx.x];
    __syncthreads();
    const long long o = ((long long)blockIdx.x * CLOUD_NT + threadIdx.x) * V;
    if (o >= n) return;
    unsigned lo[V], ok[V];
    for (int j = 0; j < V; ++j) lo[j] = FOCUS_NOT_PASSING, ok[j] = 0;
    for (int b = 0; b < nb; ++b) {
        const unsigned* p = rows + (size_t)(b0 + b) * n + o;
        unsigned key[V];
        if (V == 4) {
            const uint4 q = *reinterpret_cast<const uint4*>(p);
            key[0] = q.x; key[1] = q.y; key[2] = q.z; key[3] = q.w;
        } else {
            key[0] = *p;
        }
        for (int j = 0; j < V; ++j) {
            lo[j] = min(lo[j], key[j]);
            ok[j] |= key[j] <= bar[b];
        }
    }
    for (int j = 0; j < V; ++j) {
        atomicMin(&best[o + j], lo[j]);
        if (ok[j]) atomicOr(&pass[o + j], 1u);
    }
}

// sel [n]: what the final selection orders by
__global__ __launch_bounds__(CLOUD_NT) void k_focus_path_words(const unsigned* __restrict__ best, const unsigned* __restrict__ pass, int n,
                                                               unsigned* __restrict__ sel) {
    const int o = blockIdx.x * CLOUD_NT + threadIdx.x;
    if (o < n) sel[o] = pass[o] ? best[o] : FOCUS_NOT_PASSING;
}

}  // namespace

void omds_launch_focus_keys(hipStream_t s, const float* d, const float* vel, int dims, float lookahead, int n, unsigned* keys) {
    hipLaunchKernelGGL(k_focus_keys, dim3((n + CLOUD_NT - 1) / CLOUD_NT), dim3(CLOUD_NT), 0, s, d, vel, dims, lookahead, n, keys);
}

void omds_launch_focus_select(hipStream_t s, const unsigned* keys, int n, int n_closest, float margin, bool all_pass, int max_keep, unsigned* res) {
    hipLaunchKernelGGL(k_focus_select<false>, dim3(1), dim3(FOCUS_NT), 0, s, keys, n, n_closest, margin, all_pass ? 1 : 0, max_keep, res);
}

void omds_launch_focus_path_chunk(hipStream_t s, float* rows, const float* vel, int dims, const float* time, int C, int n, int n_closest, float margin,
                                  bool all_pass, unsigned* bars, unsigned* best, unsigned* pass) {
    unsigned* keys = reinterpret_cast<unsigned*>(rows);
    const int slices = (C + PATH_ROWS - 1) / PATH_ROWS;
    hipLaunchKernelGGL(k_focus_path_keys, dim3((n + CLOUD_NT - 1) / CLOUD_NT, slices), dim3(CLOUD_NT), 0, s, keys, vel, dims, time, C, n);
    if (!all_pass) hipLaunchKernelGGL(k_focus_path_bars, dim3(C), dim3(FOCUS_NT), 0, s, keys, n, n_closest, margin, bars);
    if (n % 4 == 0)
        hipLaunchKernelGGL(k_focus_path_merge<4>, dim3((n / 4 + CLOUD_NT - 1) / CLOUD_NT, slices), dim3(CLOUD_NT), 0, s, keys, bars, all_pass ? 1 : 0, C, n,
                           best, pass);
    else
        hipLaunchKernelGGL(k_focus_path_merge<1>, dim3((n + CLOUD_NT - 1) / CLOUD_NT, slices), dim3(CLOUD_NT), 0, s, keys, bars, all_pass ? 1 : 0, C, n,
                           best, pass);
}

void omds_launch_focus_path_select(hipStream_t s, const unsigned* best, const unsigned* pass, int n, int n_closest, int max_keep, unsigned* sel,
                                   unsigned* res) {
    hipLaunchKernelGGL(k_focus_path_words, dim3((n + CLOUD_NT - 1) / CLOUD_NT), dim3(CLOUD_NT), 0, s, best, pass, n, sel);
    hipLaunchKernelGGL(k_focus_select<true>, dim3(1), dim3(FOCUS_NT), 0, s, sel, n, n_closest, 0.f, 0, max_keep, res);
}
