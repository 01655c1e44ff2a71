// hashrng.h -- the counter-based uniform draw of the dropout masks, written once (head.hip, voxconv.hip).
//
// A mask element is a hash of (seed, step counter, layer tag, element index): rng_state = {seed, counter} lives on the device (int64[2]), so a
// captured hipGraph draws fresh masks on every replay.  tests/test_gpu_head.py pins the masks this function yields.
#pragma once
#include "common.h"

namespace papc {

__device__ __forceinline__ float hash_uniform(uint64_t seed, uint64_t counter, uint32_t tag, uint32_t idx)
{
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (counter + 1) + ((uint64_t)tag << 40) + idx;   // splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(uint32_t)(z >> 40) * (1.0f / 16777216.0f);   // 24 bits -> [0,1)
}

}  // namespace papc
