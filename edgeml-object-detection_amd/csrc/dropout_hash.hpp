// The counter hash behind every dropout mask (estimator.hip's MLP and convnet.hip's conv net).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace edgedet {

__host__ __device__ __forceinline__ uint32_t mlp_hash(uint64_t a, uint64_t b) {  // splitmix64 finalizer
    uint64_t z = a * 0x9E3779B97F4A7C15ull + b + 0x632BE59BD9B4E019ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}

// u in [0, 1) with 24 bits; a unit is kept when u >= p (probability 1 - p)
__host__ __device__ __forceinline__ bool hash_keep(uint32_t h, float p) {
    return (float)(h >> 8) * (1.0f / 16777216.0f) >= p;
}

}  // namespace edgedet
