// lanczos_table.cpp: the per-axis Lanczos3 table, host only (no HIP in that unit: it is built by g++)
#pragma once
#include <cstdint>

#include "../../include/matrix_eyes_hip_ops.h"

namespace me {
// number of weights of the (len_in, len_out) table, -1 for a length outside [1, ME_RESIZE_MAX_DIM]
int64_t lanczos3_table_weights(int32_t len_in, int32_t len_out);
// left[len_out], count[len_out] and the normalised weights of output index 0, 1, ... one after the other
void lanczos3_table_fill(int32_t len_in, int32_t len_out, int32_t* left, int32_t* count, float* weights);
}  // namespace me
