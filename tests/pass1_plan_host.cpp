// Stand-alone host build of pass 1's launch plan (optimalmodulationds_amd/csrc/pass1_plan_def.h, and pass 2's carve of
// tail_plan_def.h) for tests/test_pass1_plan_cpu.py, which compiles it with g++ -fsanitize=address,undefined and runs it on its cases:
// the header's functions are the ones the launchers launch by and the kernels call, only the compiler differs.
//   pass1_plan_host IN OUT
// IN : int32 n_cases, then per case six int32: kind, a, b, c, d, e
// OUT: per case int64 words
//   kind 0 (the natural-order grid; total, compact): pass1_size, pass1_big_tiles, then pass1_grid: big_rows, small_rows, n_big, n_small
//   kind 1 (the inverse rule; n_big, b0, count): per workgroup b0 <= b < b0 + count two words: rows, row0 of pass1_mixed_tile(b, n_big)
//   kind 2 (the block grid; N, O): ncb, nrb16, n_big, n_small, then per workgroup five words: big, r0, o0, nr, no of pass1_block
//   kind 3 (the LDS size of every launch; nhid): pass1_dmin_lds_bytes of 16, 32, 64; mixed; dyn; pass1_emit_lds_bytes of (16, nhid), (32, nhid);
//          pass1_emit_lds_max_bytes of 16, 32; exact_lds_bytes(nhid - 1); audit_lds_bytes; small_lds_bytes of (nhid, 16), (nhid, 32), (P1_MAX_NHID, 16),
//          (P1_MAX_NHID, 32); TailLdsPlan::pass2_bytes of nhid, P1_MAX_NHID
//   kind 4 (the carves; MT, nhid): Pass1Lds(MT, nhid): Hs, rowRad, rowIdx, maskS, end; Pass1DynLds(MT): Hs, rowRad, slotT, slotO, aliveS, idsS, end
//   kind 5 (the emitting launch; total): pass1_emit_ok, pass1_size, PASS1_EMIT_MAX_PAIRS
//   kind 6 (pass 2's carve; nhid): TailLdsPlan(nhid, false): Hs, gf, maskL, rowT, rowO, rowMin, gx
//   kind 7 (the small scene; plain_relu, n_dof, O, k): small_rollouts on 16 rows, on 32 rows, small_tile_rows
#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/pass1_plan_def.h"
#include "../optimalmodulationds_amd/csrc/tail_plan_def.h"

static void put(FILE* out, long long v) {
    const int64_t w = v;
    fwrite(&w, 8, 1, out);
}

int main(int argc, char** argv) {
    return run_cases(argc, argv, "pass1_plan_host", [](FILE* in, FILE* out) {
        int32_t c[6];
        if (!get(in, c, 6)) return false;
        if (c[0] == 0) {
            if (c[1] < 1) return false;
            const Pass1Grid g = pass1_grid(c[1], c[2] != 0);
            for (long long v : {(long long)pass1_size(c[1]), pass1_big_tiles(c[1]), (long long)g.big_rows, (long long)g.small_rows, g.n_big, g.n_small}) put(out, v);
        } else if (c[0] == 1) {
            for (int b = c[2]; b < c[2] + c[3]; ++b) {
                const Pass1Tile t = pass1_mixed_tile(b, c[1]);
                put(out, t.rows); put(out, t.row0);
            }
        } else if (c[0] == 2) {
            const int N = c[1], O = c[2];
            if (N < 1 || O < 1) return false;
            const Pass1BlockGrid g = pass1_block_grid(N, O);
            for (long long v : {(long long)g.ncb, (long long)g.nrb16, g.n_big, g.n_small}) put(out, v);
            for (long long wg = 0; wg < g.workgroups(); ++wg) {
                const Pass1Block k = pass1_block((unsigned)wg, (int)g.n_big, g.nrb16, (unsigned)g.ncb, N, O, [&](unsigned b) { return b / (unsigned)g.ncb; });
                for (int v : {(int)k.big, k.r0, k.o0, k.nr, k.no}) put(out, v);
            }
        } else if (c[0] == 3) {
            const int nhid = c[1];
            for (size_t v : {pass1_dmin_lds_bytes(16), pass1_dmin_lds_bytes(32), pass1_dmin_lds_bytes(64), pass1_mixed_lds_bytes(), pass1_dyn_lds_bytes(),
                             pass1_emit_lds_bytes(16, nhid), pass1_emit_lds_bytes(32, nhid), pass1_emit_lds_max_bytes(16), pass1_emit_lds_max_bytes(32),
                             exact_lds_bytes(nhid - 1), audit_lds_bytes(), small_lds_bytes(nhid, 16), small_lds_bytes(nhid, 32),
                             small_lds_bytes(P1_MAX_NHID, 16), small_lds_bytes(P1_MAX_NHID, 32), TailLdsPlan::pass2_bytes(nhid),
                             TailLdsPlan::pass2_bytes(P1_MAX_NHID)})
                put(out, (long long)v);
        } else if (c[0] == 4) {
            const Pass1Lds p(c[1], c[2]);
            const Pass1DynLds d(c[1]);
            for (int v : {p.Hs, p.rowRad, p.rowIdx, p.maskS, p.end, d.Hs, d.rowRad, d.slotT, d.slotO, d.aliveS, d.idsS, d.end}) put(out, v);
        } else if (c[0] == 5) {
            put(out, pass1_emit_ok(c[1])); put(out, (long long)pass1_size(c[1])); put(out, PASS1_EMIT_MAX_PAIRS);
        } else if (c[0] == 6) {
            const TailLdsPlan o(c[1], false);
            for (int v : {o.Hs, o.gf, o.maskL, o.rowT, o.rowO, o.rowMin, o.gx}) put(out, v);
        } else if (c[0] == 7) {
            put(out, small_rollouts(c[1] != 0, c[2], c[3], c[4], 16)); put(out, small_rollouts(c[1] != 0, c[2], c[3], c[4], 32));
            put(out, small_tile_rows(c[1] != 0, c[2], c[3], c[4]));
        } else {
            return false;
        }
        return true;
    });
}
