// Test hook (include/omds_test.h, libomds_hip_test.so only: the Makefile links this file into no other library): the top-k selection
// on caller-supplied rows, through the production launcher omds_launch_topk (k_topk and topk_row of topk_device.h as shipped), for
// tests/test_gpu_topk.py.
#include "omds_internal.h"
#include "omds_test.h"

#define HCK(expr) do { if ((expr) != hipSuccess) { rc = OMDS_ERR_HIP; goto done; } } while (0)

extern "C" OMDS_API int omds_test_topk(const float* rows, int B, int O, int k, int32_t* idx_out) {
    if (B < 1 || O < 1 || k < 1 || k > O || B > 1 << 16 || O > 1 << 20 || !rows || !idx_out) return OMDS_ERR_INVALID_ARG;
    int rc = OMDS_OK;
    float* d_rows = nullptr;
    int32_t* d_idx = nullptr;
    const size_t row_bytes = (size_t)B * O * sizeof(float), idx_bytes = (size_t)B * k * sizeof(int32_t);
    HCK(hipMalloc(&d_rows, row_bytes));
    HCK(hipMalloc(&d_idx, idx_bytes));
    HCK(hipMemcpy(d_rows, rows, row_bytes, hipMemcpyHostToDevice));
    HCK(hipMemset(d_idx, 0xFF, idx_bytes));   // -1 everywhere: a position the kernel leaves out shows
    omds_launch_topk(0, d_rows, B, O, k, d_idx);
    HCK(hipGetLastError());
    HCK(hipMemcpy(idx_out, d_idx, idx_bytes, hipMemcpyDeviceToHost));
done:
    if (d_rows) (void)hipFree(d_rows);
    if (d_idx) (void)hipFree(d_idx);
    return rc;
}
#undef HCK
