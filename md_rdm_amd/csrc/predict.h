// internal launcher of the fused predict tail (predict.hip); the C entry rdm_predict_tail_f32 lives in api.hip
#pragma once
#include "rdm_common.h"

namespace rdm {

// rows of the output are split over `split` workgroups per image (a power of two <= 2^n_out)
int predict_tail_default_split(int batch, int n_out);
int launch_predict_tail(const float* logits, const float* w, double* log_map, int64_t* decode, float* lin_map, int B, int K, int n, int n_out, int split,
                        hipStream_t stream);

}  // namespace rdm
