// common.hpp -- launch geometry and object sizes shared by the device and host
// sides.
#pragma once

#include <cstddef>
#include <cstdint>

namespace lifeapi_impl {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ULL;
// bytes of a LifeState, a LifeWeld (4 planes) and a LifeStable (10 planes)
constexpr size_t kStateBytes = 512, kWeldBytes = 4 * kStateBytes, kStableBytes = 10 * kStateBytes;

}  // namespace lifeapi_impl
