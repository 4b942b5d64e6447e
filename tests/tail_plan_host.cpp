// Stand-alone host build of the fused tails' plan (optimalmodulationds_amd/csrc/tail_plan_def.h) for tests/test_tail_plan_cpu.py,
// which compiles it with g++ -fsanitize=address,undefined and runs it on its cases: the header's functions are the ones
// tail_kernel.hip launches by, only the compiler differs.
//   tail_plan_host IN OUT
// IN : int32 n_cases, then per case nine int32: kind, n_dof, act, plain, frame, forced, ncu, k, N
// OUT: per case eight int32
//   kind 0 (a launch): index of the key omds_launch_tail looks up in TAIL_KEYS (-1: none) and its rows, the same two for
//          omds_launch_tail_sel, omds_tail_rows and tail_sel_rows with g4_ok = (act is ReLU and plain), omds_tail_scratch_rows(N, k),
//          frame_rows(4, k)
//   kind 1 (the LDS block, N = nhid): TailLdsPlan::bytes(nhid, false), (nhid, true), then of TailLdsPlan(nhid, true) in BYTES: the offsets of
//          maskL, rowT, gx, sel, its end, and the end of TailLdsPlan(nhid, false)
//   kind 2 (the table, N = i): TAIL_N_KEYS, then n_dof, act, rows, frame of TAIL_KEYS[i] (-1 each past the end), three zeros
#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/tail_plan_def.h"

int main(int argc, char** argv) {
    return run_cases(argc, argv, "tail_plan_host", [](FILE* in, FILE* out) {
        int32_t c[9];
        if (!get(in, c, 9)) return false;
        const int32_t kind = c[0], n_dof = c[1], act = c[2], plain = c[3], frame = c[4], forced = c[5], ncu = c[6], k = c[7], N = c[8];
        int32_t row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (kind == 0) {
            if (k < 1 || N < 1 || ncu < 1) return false;
            const TailKey kt = tail_plan_key(n_dof, act, plain != 0, frame != 0, N, k, ncu, forced);
            const TailKey ks = tail_sel_plan_key(n_dof, act, plain != 0, frame != 0, N, k, ncu, forced);
            row[0] = tail_key_index(kt);
            row[1] = kt.rows;
            row[2] = tail_key_index(ks);
            row[3] = ks.rows;
            const bool g4_ok = act == OMDS_ACT_RELU && plain != 0;
            row[4] = omds_tail_rows(N, k, g4_ok, ncu, forced);
            row[5] = tail_sel_rows(N, k, g4_ok, ncu, forced);
            row[6] = omds_tail_scratch_rows(N, k);
            row[7] = frame_rows(4, k);
        } else if (kind == 1) {
            const TailLdsPlan with(N, true), without(N, false);
            row[0] = (int32_t)TailLdsPlan::bytes(N, false);
            row[1] = (int32_t)TailLdsPlan::bytes(N, true);
            row[2] = 4 * with.maskL; row[3] = 4 * with.rowT; row[4] = 4 * with.gx; row[5] = 4 * with.sel;
            row[6] = 4 * with.end; row[7] = 4 * without.end;
        } else if (kind == 2) {
            const bool in_table = N >= 0 && N < TAIL_N_KEYS;
            row[0] = TAIL_N_KEYS;
            row[1] = in_table ? TAIL_KEYS[N].n_dof : -1;
            row[2] = in_table ? TAIL_KEYS[N].act : -1;
            row[3] = in_table ? TAIL_KEYS[N].rows : -1;
            row[4] = in_table ? (int32_t)TAIL_KEYS[N].frame : -1;
        } else {
            return false;
        }
        fwrite(row, 4, 8, out);
        return true;
    });
}
