// acf_neumf_adam.h — the dense Keras 2.2 Adam of libacf_neumf.so for its other units (acf_keras_mf.hip).
// After hip_runtime.h, acf_neumf.h.  k_nmf_adam and this function's one definition are in acf_neumf.hip.
#pragma once

// Iteration t over the n4 float4s of p, g, m, v on stream s: lr_t from adam_lr_t, g zeroed behind the stream.
__attribute__((visibility("hidden"))) int acf_dense_adam(float* p, float* g, float* m, float* v, int64_t n4,
                                                         int64_t t, const acf_neumf_hparams* hp, hipStream_t s);
