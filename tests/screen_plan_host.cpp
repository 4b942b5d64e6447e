// Stand-alone host build of the screened step's launch plan (optimalmodulationds_amd/csrc/screen_plan_def.h) for
// tests/test_screen_plan_cpu.py, which compiles it with g++ -fsanitize=address,undefined and runs it on its cases: the header's
// functions are the ones screen_kernel.hip / screen_exact.hip launch by and their kernels call, only the compiler differs.
//   screen_plan_host IN OUT
// IN : int32 n_cases, then per case six int32: kind, a, b, c, d, e
// OUT: per case int64 words
//   kind 0 (a k_screen launch; B, O, nhh, ncu, want_select): selects, unit, units_base, units_rem, grid, res_tiles, lds_bytes,
//          lds_max_bytes, total, omds_screen_can_select(O); then per workgroup w < grid three words: p0, p1, tiles of ScreenLaunchPlan::chunk(w)
//   kind 1 (the audit rounds; n, G, cap): audit_grid(cap), full, rest0, rest, last64; then per workgroup w < G two words: in_last(w), last_row0(w)
//   kind 2 (the LDS of k_exact / k_audit; nhh): exact_lds_bytes(nhh), audit_lds_bytes(), omds_screen_lds_bytes(nhh), and the geometry:
//          SC_WAVES, SC_NT, SC_ROWS, SC_SLICE, SC_RING, SC_DIST, SC_PW, SC_MAX_TILES, SEL_WAVES, EXACT_RESIDENT
#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/screen_plan_def.h"

static void put(FILE* out, long long v) {
    const int64_t w = v;
    fwrite(&w, 8, 1, out);
}

int main(int argc, char** argv) {
    return run_cases(argc, argv, "screen_plan_host", [](FILE* in, FILE* out) {
        int32_t c[6];
        if (!get(in, c, 6)) return false;
        if (c[0] == 0) {
            const int B = c[1], O = c[2], nhh = c[3], ncu = c[4];
            if (B < 1 || O < 1 || ncu < 1) return false;
            const ScreenLaunchPlan p = screen_plan(B, O, nhh, ncu, c[5] != 0);
            for (long long v : {(long long)p.selects, (long long)p.unit, (long long)p.units_base, (long long)p.units_rem, (long long)p.grid, (long long)p.res_tiles,
                                (long long)p.lds_bytes, (long long)p.lds_max_bytes, p.total, (long long)omds_screen_can_select(O)})
                put(out, v);
            for (int w = 0; w < p.grid; ++w) {
                const ScreenChunk ch = p.chunk(w);
                put(out, ch.p0); put(out, ch.p1); put(out, ch.tiles());
            }
        } else if (c[0] == 1) {
            const int n = c[1], G = c[2], cap = c[3];
            if (n < 0 || G < 1) return false;
            const AuditRounds ar = audit_rounds(n, G);
            for (long long v : {(long long)audit_grid(cap), (long long)ar.full, (long long)ar.rest0, (long long)ar.rest, (long long)ar.last64}) put(out, v);
            for (int w = 0; w < G; ++w) { put(out, ar.in_last((unsigned)w)); put(out, ar.last_row0((unsigned)w)); }
        } else if (c[0] == 2) {
            for (long long v : {(long long)exact_lds_bytes(c[1]), (long long)audit_lds_bytes(), (long long)omds_screen_lds_bytes(c[1]), (long long)SC_WAVES,
                                (long long)SC_NT, (long long)SC_ROWS, (long long)SC_SLICE, (long long)SC_RING, (long long)SC_DIST, (long long)SC_PW,
                                (long long)SC_MAX_TILES, (long long)SEL_WAVES, (long long)EXACT_RESIDENT})
                put(out, v);
        } else {
            return false;
        }
        return true;
    });
}
