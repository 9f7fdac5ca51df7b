// ptmi_hd.h - PTMI_HD: what stands in front of a function that the host, the kernels and the serial models of the tests
// compile from one copy (bvh_build_common.h, leaf_cull.h, scene_refit_common.h, the reference helpers of ptmi_internal.h).
#ifndef PTMI_HD_H
#define PTMI_HD_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PTMI_HD __host__ __device__ __forceinline__
#else
#define PTMI_HD inline
#endif

#endif  // PTMI_HD_H
