// va_scan.h -- the integer sums and prefix sums over a wave and over a workgroup that the kernel files share
// ("Scans").  Device code only.  Every T is an integer type: two's-complement addition is associative,
// so the results do not depend on the order in which the lanes' values meet.
#pragma once
#include "va_common.h"

namespace va {

// the sum of v over the 64 lanes of the wave, in every lane.  Every lane of the wave calls it.
template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1)
        v += __shfl_xor(v, d, kWave);
    return v;
}

// the sum of v over the lanes 0 .. lane of the wave (lane = threadIdx.x % 64).  Every lane of the wave calls it.
template <class T>
__device__ __forceinline__ T wave_inclusive(T v, int lane)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T u = __shfl_up(v, d, kWave);
        if (lane >= d)
            v += u;
    }
    return v;
}

// The exclusive prefix of v over the threads of the workgroup, in threadIdx.x order; total: the workgroup's sum, in
// every lane.  WAVES is the number of waves of the workgroup; WAVES = 0 takes it from blockDim.x.
//   - Every thread of the workgroup calls it (it holds barriers), with the same `part`.
//   - blockDim.x is a multiple of 64 and at most 1024; `part` is LDS with an entry per wave.
//   - The first barrier retires whoever still reads `part` from an earlier call, the second follows the write of
//     `part`: calls may follow one another on the same `part` with no barrier of the caller's between them.
//   - What stays with the caller: a barrier before other threads read LDS that the caller itself wrote.  The two
//     barriers in here order `part` alone; that they also order a caller's LDS is not part of the contract.
template <int WAVES, class T>
__device__ __forceinline__ T block_exclusive(T v, T *part, T &total)
{
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int nwaves = WAVES ? WAVES : (int)blockDim.x / kWave;
    const T incl = wave_inclusive(v, lane);
    __syncthreads();
    if (lane == kWave - 1)
        part[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < nwaves; k++) {
        const T s = part[k];
        before += k < wave ? s : (T)0;
        all += s;
    }
    total = all;
    return before + incl - v;
}

}  // namespace va
