// Stand-alone host build of the trainer's route and split policy (optimalmodulationds_amd/csrc/train_plan_def.h) for
// tests/test_train_plan_cpu.py, which compiles it with g++ -fsanitize=address,undefined and runs it on its cases: the header's
// functions are the ones train.hip calls, only the compiler differs.
//   train_plan_host IN OUT
// IN : int32 n_cases, then per case: int32 general (the "general kernel everywhere" flag), int32 L, int32 B, int32 dims[L + 1]
// OUT: per case and layer i < L nine int32: forward, wgrad, wgrad_tt, inputgrad (TrainRoute), splits, kchunk, the rows of the last
//      chunk, rsplit, rows_per -- the split numbers with the partial-sum buffer a trainer of these dims allocates
// dims and the plan are allocated at exactly L + 1 and L elements, so that a read or write past either is the sanitizer's to report.
#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/train_plan_def.h"

int main(int argc, char** argv) {
    return run_cases(argc, argv, "train_plan_host", [](FILE* in, FILE* out) {
        int32_t general = 0, L = 0, B = 0;
        if (!get(in, &general) || !get(in, &L) || !get(in, &B) || L < 1 || B < 1) return false;
        int32_t* dims = exactly<int32_t>((size_t)L + 1);
        TrainLayerPlan* plan = exactly<TrainLayerPlan>((size_t)L);
        if (!get(in, dims, (size_t)L + 1)) return false;
        train_plan_layers(dims, L, general != 0, plan);
        const size_t partial_floats = train_partial_floats(dims, L);
        for (int i = 0; i < L; ++i) {
            const TrainSplit t = train_plan_split(B, dims[i], dims[i + 1], partial_floats);
            const int32_t row[9] = {plan[i].forward, plan[i].wgrad, plan[i].wgrad_tt, plan[i].inputgrad, t.splits, t.kchunk,
                                    B - (t.splits - 1) * t.kchunk, t.rsplit, (int32_t)t.rows_per};
            fwrite(row, 4, 9, out);
        }
        free(dims);
        free(plan);
        return true;
    });
}
