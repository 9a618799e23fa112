// Host-side pieces the weight-gradient translation units share (gemm.hip defines them, wgrad_f16x3.hip uses them).
// Internal: plain C++ with hidden visibility, nothing here is part of the C ABI (include/upnerf_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include "upnerf_hip.h"

#define WG_CHUNK 32  // rows per staged chunk of the fp32 kernel; upnerf_wgrad and upnerf_wgrad16 round a split's rows to it

namespace upnerf_host __attribute__((visibility("hidden"))) {

// block shape of an N x K weight gradient (each side 64, 128 or 256): what the slab layout and the reduction are cut by
void wgrad_shape(int N, int K, int* TN, int* TK);
// the record of a problem whose slabs are written but not summed (n2 / vslabs fields left empty)
upnerf_wgrad_pending reduce_desc(int N, int K, int TN, int TK, int nsplit, const float* slabs, const float* bslabs, float* dW, int ldo,
                                 float* db);
// dW / db (/ dW2 / db2 / dv / dbv) = fixed-order sum of the slabs P describes, as a launch of its own
void launch_reduce(hipStream_t st, const upnerf_wgrad_pending& P);

}  // namespace upnerf_host
