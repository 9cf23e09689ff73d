// Source index of NEAREST_EXACT resampling (ATen's nearest_exact_idx with scale = (float)in / (float)out): shared by the resize kernel of
// prepost.hip and the ensembling gather of ensemble.hip, so the two cannot drift apart (tests/test_prepost_gpu.py pins it to the host recipe).
#pragma once
#include <hip/hip_runtime.h>

// src = min(floor((dst + 0.5) * in / out), in - 1)
__device__ __forceinline__ int nearest_exact_src(int dst, float scale, int in) { return min((int)floorf(((float)dst + 0.5f) * scale), in - 1); }
