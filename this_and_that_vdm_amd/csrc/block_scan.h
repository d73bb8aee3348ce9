// Integer-style sums and prefix sums over a wave and over a workgroup of WAVES waves of 64 lanes, in thread order: the pieces the image
// codecs, the tensor statistics and the frame metrics build their reductions and scans from.  Device only; every lane of the workgroup
// calls the block_* functions together.  (The floating-point reductions of the norm, elementwise, image, attention and GEMM units are
// butterflies with barriers of their own and are not built from these.)
#pragma once

// lane 0 gets the wave's sum.  A fixed tree: the same bits every time, doubles included
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// the inclusive prefix sum over the wave's lanes
template <typename T> __device__ __forceinline__ T wave_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T a = __shfl_up(v, o, 64);
    if (lane >= o) v += a;
  }
  return v;
}

// the sum of `mine` over the threads before this one, and over all of them in `total`.  red_s: WAVES values of LDS.  Holds exactly one
// __syncthreads, which also orders whatever the caller stored before the call.  The caller's duty: a barrier before red_s is written again.
template <int WAVES, typename T> __device__ __forceinline__ T block_scan_excl(T mine, T* red_s, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T incl = wave_scan(mine);
  if (lane == 63) red_s[wave] = incl;
  __syncthreads();
  T before = incl - mine;
  total = 0;
  for (int wv = 0; wv < WAVES; ++wv) {
    if (wv < wave) before += red_s[wv];
    total += red_s[wv];
  }
  return before;
}

// the sum of `mine` over the workgroup, in every thread; red_s, its one __syncthreads and the caller's duty as for block_scan_excl
template <int WAVES, typename T> __device__ __forceinline__ T block_sum(T mine, T* red_s) {
  const T s = wave_sum(mine);
  if ((threadIdx.x & 63) == 0) red_s[threadIdx.x >> 6] = s;
  __syncthreads();
  T total = 0;
  for (int wv = 0; wv < WAVES; ++wv) total += red_s[wv];
  return total;
}

// an exclusive scan of v[0 .. count) in place by one workgroup, 64 WAVES values a pass with the carry of the passes before; returns the sum
template <int WAVES, typename T> __device__ __forceinline__ T scan_in_place(T* __restrict__ v, long long count, T* red_s) {
  T carry = 0;
  for (long long at = 0; at < count; at += WAVES * 64) {
    const long long i = at + threadIdx.x;
    T all;
    const T before = carry + block_scan_excl<WAVES>(i < count ? v[i] : (T)0, red_s, all);
    if (i < count) v[i] = before;
    carry += all;
    __syncthreads();
  }
  return carry;
}
