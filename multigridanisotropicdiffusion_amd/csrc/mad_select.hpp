// mad_select.hpp -- exact selection on the GPU: the k-th smallest (0-based) of n non-negative
// IEEE values, by a most-significant-digit radix select on their bit patterns (non-negative
// floats and doubles order as unsigned integers).  Used by the Perona-Malik contrast quantile
// (include/mad_pm.h, "Contrast from a quantile").
//
// Keys are uint32_t (float) or uint64_t (double); a digit is kSelBits = 11 bits, the last one
// what remains (fp32: 11 + 11 + 10, three digits; fp64: 5 x 11 + 9, six).  Per digit, most
// significant first:
//   sel_hist_k   counts, per workgroup in LDS, the digit of every key that matches the prefix
//                found so far, and adds its non-zero bins to the digit's global histogram with
//                integer atomics
//   sel_scan_k   one workgroup: scans the 2048 merged counts, finds the bin that holds the
//                remaining rank, appends the digit to the prefix and takes the counts below it
//                off the rank, all in device memory
// After the last digit the prefix is the key.  The order between the phases is the order of
// the kernels on one stream; no kernel waits for another workgroup, and all counts are
// integers, so the result does not depend on the schedule: it is bit-exact and the same in
// every run.
//
// Compaction.  Every workgroup reads one contiguous chunk of the keys, the same chunk in every
// pass.  From kSelListMin keys on, the histogram pass of the second digit also copies the keys
// that match the first digit to the front of the workgroup's own chunk of a candidate list (slots
// drawn from an LDS counter, one draw per wave) and records how many it kept; the later digits
// read those segments instead of the source.  Only the multiset matters, so the order inside a
// segment is free, and no global atomic is involved.  The list holds n keys, so n equal keys
// fit, and every pass still reads each of its inputs once: the pass count is the digit count
// whatever the data.  Below kSelListMin every digit reads the source; the result is the same.
//
// Counts are uint32_t: n < 2^32 is the caller's to ensure.  Every selection starts by zeroing all
// histograms, the segment counts and the state, so nothing is left from the last.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace mad {

constexpr int kSelBits = 11;
constexpr int kSelBins = 1 << kSelBits;
constexpr int kSelMaxDigits = 6;
constexpr int64_t kSelListMin = 65536;
constexpr int kSelItems = 4;  // keys per thread and loop trip of sel_hist_k

constexpr int kSelMaxBlocks = 2048;

// device state of one selection
struct SelState {
  unsigned long long prefix;  // the digits found so far, in place
  unsigned long long rank;    // the rank that remains among the keys matching the prefix
  double value;               // the selected value (set by the last digit's scan)
};

template <typename K>
__device__ inline double sel_key_value(K key);
template <>
__device__ inline double sel_key_value<uint32_t>(uint32_t key) {
  return (double)__uint_as_float(key);
}
template <>
__device__ inline double sel_key_value<uint64_t>(uint64_t key) {
  return __longlong_as_double((long long)key);
}

// Histogram of the digit at [shift, shift + bits) over the keys that agree with st->prefix
// above it (first: no prefix yet, every key counts).  Workgroup b works on the chunk
// [b chunk, min(n, (b + 1) chunk)) of src, or, with from_list, on the first counts[b] keys of its
// chunk of the candidate list (src = the list then).  list (may be null): every counted key is
// copied to the front of the workgroup's chunk of it and counts[b] is set.
// Block = 256 threads, 256 * kSelItems keys per trip; chunk is a multiple of that.
template <typename K>
__global__ void __launch_bounds__(256) sel_hist_k(const K* __restrict__ src, unsigned long long n,
                                                  unsigned long long chunk, int from_list,
                                                  const SelState* __restrict__ st, int shift, int bits, int first,
                                                  unsigned int* __restrict__ hist, K* __restrict__ list,
                                                  unsigned int* __restrict__ counts) {
  __shared__ unsigned int h[kSelBins];
  __shared__ unsigned int kept;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  for (int b = tid; b < kSelBins; b += 256) h[b] = 0u;
  if (tid == 0) kept = 0u;
  __syncthreads();
  const unsigned long long lo = blockIdx.x * chunk;
  const unsigned long long hi = from_list ? lo + counts[blockIdx.x] : (lo + chunk < n ? lo + chunk : n);
  const K want = first ? K(0) : (K)(st->prefix >> (shift + bits));
  const unsigned int dmask = (1u << bits) - 1u;
  for (unsigned long long i0 = lo; i0 < hi; i0 += 256ull * kSelItems) {
    K key[kSelItems];
    bool ok[kSelItems];
#pragma unroll
    for (int j = 0; j < kSelItems; ++j) {
      const unsigned long long i = i0 + 256ull * j + tid;
      ok[j] = i < hi;
      key[j] = ok[j] ? src[i] : K(0);
    }
#pragma unroll
    for (int j = 0; j < kSelItems; ++j) {
      // (key >> shift) >> bits: two shifts, so the first digit's shift + bits = the key width is defined
      const bool hit = ok[j] && (first || (K)((key[j] >> shift) >> bits) == want);
      const unsigned int d = (unsigned int)(key[j] >> shift) & dmask;
      // the loop is uniform over the block, so every lane of the wave votes
      const unsigned long long act = __ballot(hit);
      if (act) {
        const int lead = __ffsll((long long)act) - 1;
        const unsigned int d0 = (unsigned int)__shfl((int)d, lead);
        // one add per wave where all its keys share the digit (flat regions, a constant image)
        if (__ballot(hit && d == d0) == act) {
          if (lane == lead) atomicAdd(&h[d0], (unsigned int)__popcll(act));
        } else if (hit) {
          atomicAdd(&h[d], 1u);
        }
        if (list) {
          unsigned int base = 0;
          if (lane == lead) base = atomicAdd(&kept, (unsigned int)__popcll(act));
          base = (unsigned int)__shfl((int)base, lead);
          if (hit) list[lo + base + __popcll(act & ((1ull << lane) - 1ull))] = key[j];
        }
      }
    }
  }
  __syncthreads();
  for (int b = tid; b < kSelBins; b += 256) {
    const unsigned int c = h[b];
    if (c) atomicAdd(&hist[b], c);
  }
  if (list && tid == 0) counts[blockIdx.x] = kept;
}

// One workgroup of 256 threads, eight bins each: finds the bin holding the rank (rank0 with
// first, else st->rank), st->prefix |= bin << shift, st->rank -= the counts below the bin.
// last: st->value = the key's value.  The counted keys number more than the rank (the caller's
// 0 <= k < n, and each digit keeps the invariant), so exactly one thread finds its bin.
template <typename K>
__global__ void __launch_bounds__(256) sel_scan_k(const unsigned int* __restrict__ hist, SelState* __restrict__ st,
                                                  unsigned long long rank0, int shift, int bits, int first, int last) {
  __shared__ unsigned long long part[256];
  const int tid = threadIdx.x;
  const int bins = 1 << bits, per = kSelBins / 256;
  unsigned int c[kSelBins / 256];
  unsigned long long sum = 0;
#pragma unroll
  for (int j = 0; j < per; ++j) {
    const int b = tid * per + j;
    c[j] = b < bins ? hist[b] : 0u;
    sum += c[j];
  }
  part[tid] = sum;
  __syncthreads();
  // inclusive scan of the 256 partial sums
  for (int off = 1; off < 256; off <<= 1) {
    const unsigned long long add = tid >= off ? part[tid - off] : 0ull;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  const unsigned long long rank = first ? rank0 : st->rank;
  unsigned long long below = part[tid] - sum;
  __syncthreads();  // every thread has read st->rank before one of them writes it
  if (rank < below || rank >= part[tid]) return;
#pragma unroll
  for (int j = 0; j < per; ++j) {
    if (rank < below + c[j]) {
      const unsigned long long prefix = (first ? 0ull : st->prefix) | ((unsigned long long)(tid * per + j) << shift);
      st->prefix = prefix;
      st->rank = rank - below;
      if (last) st->value = sel_key_value<K>((K)prefix);
      return;
    }
    below += c[j];
  }
}

// Host side.  One scratch per context: the per-digit histograms, the per-workgroup segment
// counts and the state in one allocation, and the candidate list, grown on demand.
struct SelScratch {
  void* work = nullptr;  // kSelMaxDigits * kSelBins + kSelMaxBlocks uint32_t, then SelState
  void* list = nullptr;
  size_t list_bytes = 0;
  static constexpr size_t count_off = sizeof(unsigned int) * kSelMaxDigits * kSelBins;
  static constexpr size_t state_off = count_off + sizeof(unsigned int) * kSelMaxBlocks;
  static constexpr size_t work_bytes = state_off + sizeof(SelState);
  unsigned int* counts() const { return (unsigned int*)((char*)work + count_off); }
  SelState* state() const { return (SelState*)((char*)work + state_off); }
  const double* value() const { return &state()->value; }  // device address of the result
};

// Launches the selection of rank k among the n keys at src on stream st; the result stays in
// device memory at s.value().  The scratch must have been sized by the caller (work: work_bytes;
// list: n keys when n >= kSelListMin).  Returns the first launch error.
template <typename K>
hipError_t select_launch(const SelScratch& s, const K* src, int64_t n, int64_t k, hipStream_t st) {
  hipError_t e = hipMemsetAsync(s.work, 0, SelScratch::work_bytes, st);
  if (e != hipSuccess) return e;
  const int width = 8 * (int)sizeof(K);
  const int digits = (width + kSelBits - 1) / kSelBits;
  const bool use_list = n >= kSelListMin;
  // contiguous chunks, a multiple of one trip, at most kSelMaxBlocks of them
  const unsigned long long trip = 256ull * kSelItems, un = (unsigned long long)n;
  const unsigned long long chunk = ((un + kSelMaxBlocks - 1) / kSelMaxBlocks + trip - 1) / trip * trip;
  const unsigned int blocks = (unsigned int)((un + chunk - 1) / chunk);
  SelState* state = s.state();
  for (int d = 0; d < digits; ++d) {
    const int shift = std::max(0, width - kSelBits * (d + 1));
    const int bits = std::min(kSelBits, width - kSelBits * d);
    unsigned int* hist = (unsigned int*)s.work + (size_t)d * kSelBins;
    const bool from_list = use_list && d >= 2;
    K* list = use_list && d == 1 ? (K*)s.list : nullptr;
    hipLaunchKernelGGL((sel_hist_k<K>), dim3(blocks), dim3(256), 0, st, from_list ? (const K*)s.list : src, un, chunk,
                       from_list ? 1 : 0, state, shift, bits, d == 0 ? 1 : 0, hist, list, s.counts());
    hipLaunchKernelGGL((sel_scan_k<K>), dim3(1), dim3(256), 0, st, hist, state, (unsigned long long)k, shift, bits,
                       d == 0 ? 1 : 0, d == digits - 1 ? 1 : 0);
  }
  return hipGetLastError();
}

}  // namespace mad
