// Pieces shared by kernels_misc.hip and linear_attn.hip: vector types, loads / stores of the three activation storage types, the wave butterfly sum and the
// head geometry of both attention kinds.  Internal linkage: every translation unit gets its own copy.
#pragma once
#include "common.h"

namespace irsde {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16_t;
typedef _Float16 f16_t;
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx8 __attribute__((ext_vector_type(8)));

namespace {

// Activation storage type T (fp32, bf16 under IRSDE_FLAG_BF16_ACT, IEEE fp16 under IRSDE_FLAG_F16_ACT): arithmetic is fp32 either way.
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16_t* p) { return (float)*p; }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld4(const bf16_t* p) {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
__device__ __forceinline__ float ld1(const f16_t* p) { return (float)*p; }
__device__ __forceinline__ float4 ld4(const f16_t* p) {
    const f16x4 v = *reinterpret_cast<const f16x4*>(p);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
__device__ __forceinline__ void st1(f16_t* p, float v) { *p = (f16_t)v; }  // RNE
__device__ __forceinline__ void st4(f16_t* p, float4 v) {
    const floatx4 f = {v.x, v.y, v.z, v.w};
    *reinterpret_cast<f16x4*>(p) = __builtin_convertvector(f, f16x4);  // RNE
}
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(bf16_t* p, float v) { *p = (bf16_t)v; }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void st4(bf16_t* p, float4 v) {
    const floatx4 f = {v.x, v.y, v.z, v.w};
    *reinterpret_cast<bf16x4*>(p) = __builtin_convertvector(f, bf16x4);  // RNE
}

__device__ __forceinline__ float wave_xor_sum(float v, int width) {
    for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// LinearAttention and the denoising-sde softmax attention: qkv rows of q | k | v, 4 heads x 32 channels each
constexpr int kHeads = 4;
constexpr int kDh = 32;
constexpr int kHid = kHeads * kDh;  // 128
constexpr int kQkv = 3 * kHid;      // 384

}  // namespace
}  // namespace irsde
