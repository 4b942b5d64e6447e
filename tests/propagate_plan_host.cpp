// Stand-alone host build of the propagate's schedule (optimalmodulationds_amd/csrc/propagate_plan_def.h) for
// tests/test_propagate_plan_cpu.py, which compiles it with g++ -fsanitize=address,undefined and runs it on its cases: the header's
// function is the one propagate.hip enqueues by, only the compiler differs.
//   propagate_plan_host IN OUT
// IN : int32 n_cases, then per case seven int32: N, O, H, shared, route, flags, blocks_ok
// OUT: per case four int32: parts, split, omds_pipeline_split(N), pipeline_blocks_shape_ok(N, O)
#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/propagate_plan_def.h"

int main(int argc, char** argv) {
    return run_cases(argc, argv, "propagate_plan_host", [](FILE* in, FILE* out) {
        int32_t c[7];
        if (!get(in, c, 7)) return false;
        if (c[4] < 0 || c[4] > (int32_t)StepRoute::ScreenMatrix) return false;
        const PipelinePlan p = omds_pipeline_plan(c[0], c[1], c[2], c[3] != 0, (StepRoute)c[4], (unsigned)c[5], c[6] != 0);
        const int32_t row[4] = {p.parts, p.split, omds_pipeline_split(c[0]), (int32_t)pipeline_blocks_shape_ok(c[0], c[1])};
        fwrite(row, 4, 4, out);
        return true;
    });
}
