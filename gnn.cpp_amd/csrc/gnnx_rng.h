// The one counter-based generator of the library: the SplitMix64 finaliser and its golden-ratio increment, as the synthetic inputs
// (gnnx_synth.hip), the neighbour sampler (gnnx_sample.hip), the negative sampler (gnnx_negative.hip) and the random walks
// (gnnx_walk.hip) key their draws -- include/gnnx.h states each key.  gnn.cpp_amd/synth.py and the tests' *_ref.py restate it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gnnx {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

__host__ __device__ inline uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + kGolden;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace gnnx
