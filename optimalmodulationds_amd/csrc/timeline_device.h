// The phase-timestamp macros of the diagnostic builds (make timeline / timeline_e / VFLAGS=-DOMDS_TAIL_TL) and the k_tail_sel stamp table; every
// macro compiles to nothing in the product.  Included by the pass-1 and pass-2 headers, step_device.h and tail_kernel.hip.
#pragma once

// Diagnostic build (make timeline VFLAGS=-DOMDS_TAIL_TL, tools/tail_timeline.py): thread 0 of every k_tail_sel workgroup stamps the shader clock
// at the phase boundaries; a one-thread kernel prints the table after the launch chosen by OMDS_TAIL_TL_STEP.
#ifdef OMDS_TAIL_TL
static __device__ unsigned long long g_tail_tl[1024][20];
#define OMDS_TL_STAMP(i)                                                                                   \
    do {                                                                                                   \
        if (threadIdx.x == 0 && blockIdx.x < 1024) g_tail_tl[blockIdx.x][i] = (i) == 0 || (i) == 19 ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define OMDS_TL_STAMP(i)
#endif

// Diagnostic build (make timeline): workgroup phase timestamps, read by tools/pass1_timeline.py.  Compiles to nothing otherwise.
#ifdef OMDS_TIMELINE
#ifdef OMDS_TIMELINE_E   // per-WAVE stamps around one level's product and epilogue instead (tools/pass1_dyn_epilogue.py): [workgroup][wave][8]
#define OMDS_TL(i) do { } while (0)
#define OMDS_TLE(l, s) do { if (m.tl && (l) == OMDS_TIMELINE_E && (threadIdx.x & 63) == 0) m.tl[((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * 8 + (s)] = wall_clock64(); } while (0)
#else
#define OMDS_TL(i) do { if (m.tl && threadIdx.x == 0) m.tl[(size_t)blockIdx.x * 16 + (i)] = wall_clock64(); } while (0)
#define OMDS_TLE(l, s) do { } while (0)
#endif
#define OMDS_TL_WAIT(what) asm volatile("s_waitcnt " what ::: "memory")
// HW_ID and XCC_ID: which CU this workgroup landed on
#define OMDS_TL_HWID(i) do { if (m.tl && threadIdx.x == 0) m.tl[(size_t)blockIdx.x * 16 + (i)] = (unsigned long long)__builtin_amdgcn_s_getreg(63492) | ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32); } while (0)
#else
#define OMDS_TL_HWID(i) do { } while (0)
#define OMDS_TL(i) do { } while (0)
#define OMDS_TLE(l, s) do { } while (0)
#define OMDS_TL_WAIT(what) do { } while (0)
#endif
