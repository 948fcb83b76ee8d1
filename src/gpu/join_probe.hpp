// The join fast path's probe: one software-pipelined kernel over every table
// layout (join_fast.hip has the layouts and their build kernels).
//
// A lane takes PPIPE consecutive probe rows per batch:
//  * one validity byte per 8 rows gives the batch's live bits, the tail is
//    clipped, and a key that can never be in the table is masked out;
//  * keys, then slot indices, then ALL first-slot loads issue back to back
//    with nothing dependent between them — PPIPE outstanding random loads
//    per lane are the memory-level parallelism this kernel lives on;
//  * resolve counts each row's matches and carries the FIRST match's build
//    row in a register, so the (overwhelmingly common) exactly-one-match row
//    emits without walking its chain again;
//  * FILL: one atomicAdd per wave and batch reserves output space (a wave
//    prefix sum gives each lane its base), then plain stores; only a row
//    with several matches rescans its chain, cache-warm;
//  * count mode adds one wave sum per kernel to the counter instead.
//
// Contract, for every layout:
//  * counter receives the number of matching pairs, in both modes;
//  * pairs past out_capacity are counted and not written;
//  * build_matched (may be null) is written even at capacity 0, which is how
//    a mark-only probe runs: FILL with null outputs;
//  * pair order is unspecified;
//  * idxmap (may be null; chained layouts only) holds the source rows of
//    partitioned probe keys and replaces the row number in out_probe.
//
// A layout L is passed by value: the slot pointer, `mask` or `range`, and
// `kmin` where it has one. It supplies only what differs between the tables:
//   Tag     what a lane keeps per row to compare against slot words
//   Word    what one slot load returns
//   Index   a slot index
//   index(key, Tag&, bool& live)  first slot of a key; live = false for a key
//           that cannot be in the table (its load still has to stay inside)
//   load(idx), next(idx), reindex(Tag)  reindex gives the first slot again,
//           on the rare chain path, so that indices do not stay in registers
//   empty(Word), match(Word, Tag), chain(Word), row1(Word)
//   CHAINED       false: at most one match per key, no chain walk, no idxmap,
//                 and next, reindex and chain are not needed
//   PLAIN_BATCH   true: a batch wholly in range loads its keys unclamped, as
//                 consecutive loads the compiler merges into wide ones;
//                 false: every key load is clamped and unconditional
#pragma once
#include "srj_common.hpp"

namespace srj {

template <typename L, typename K, bool FILL, bool HAS_VALID, int PPIPE>
__global__ void join_probe_kernel_t(
    const K* __restrict__ probe, const uint8_t* __restrict__ pvalid,
    int64_t nprobe, L layout, uint64_t* __restrict__ counter,
    int32_t* __restrict__ out_build, int64_t* __restrict__ out_probe,
    int64_t out_capacity, uint8_t* __restrict__ build_matched,
    const int32_t* __restrict__ idxmap) {
  static_assert(PPIPE == 8 || PPIPE == 16, "validity bytes per batch");
  using Tag = typename L::Tag;
  using Word = typename L::Word;
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  int lane = threadIdx.x & (WAVE - 1);
  uint64_t count_local = 0;
  int64_t nbatch = (nprobe + (int64_t)PPIPE - 1) / PPIPE;
  // pad so every lane of a wave runs the same iterations (wave shuffles)
  int64_t nbatch_pad = (nbatch + WAVE - 1) & ~(int64_t)(WAVE - 1);
  for (int64_t batch = tid; batch < nbatch_pad; batch += nthreads) {
    bool batch_ok = batch < nbatch;
    int64_t base = batch_ok ? batch * PPIPE : 0;
    uint32_t vbits = (1u << PPIPE) - 1u;
    if (HAS_VALID) {
      vbits = pvalid[base >> 3];
      // the second byte of a 16-row batch may lie past the mask's last byte
      if (PPIPE == 16 && base + 8 < nprobe)
        vbits |= (uint32_t)pvalid[(base >> 3) + 1] << 8;
    }
    if (base + PPIPE > nprobe) {
      int64_t tail = nprobe - base;
      vbits &= (uint32_t)((1u << (tail < 0 ? 0 : tail)) - 1u);
    }
    if (!batch_ok) vbits = 0;
    K k[PPIPE];
    if (L::PLAIN_BATCH && base + PPIPE <= nprobe) {
#pragma unroll
      for (int b = 0; b < PPIPE; ++b) k[b] = probe[base + b];
    } else {
#pragma unroll
      for (int b = 0; b < PPIPE; ++b) {
        int64_t row = base + b;
        if (L::PLAIN_BATCH)
          k[b] = row < nprobe ? probe[row] : (K)0;  // masked by vbits
        else
          k[b] = probe[row < nprobe ? row : 0];  // clamped, unconditional
      }
    }
    Tag tag[PPIPE];
    Word fw[PPIPE];
    {
      typename L::Index s[PPIPE];
#pragma unroll
      for (int b = 0; b < PPIPE; ++b) {
        bool live;
        s[b] = layout.index((long long)k[b], tag[b], live);
        if (!live) vbits &= ~(1u << b);
      }
#pragma unroll
      for (int b = 0; b < PPIPE; ++b) fw[b] = layout.load(s[b]);
    }
    // per row: bit of `hit` = has a match, bit of `multi` = has several
    uint32_t nm = 0, hit = 0, multi = 0;
    uint32_t hit1[PPIPE];  // row + 1 of the first match
#pragma unroll
    for (int b = 0; b < PPIPE; ++b) {
      hit1[b] = 0;
      // empty first: an empty slot must not match a key whose tag is 0
      if (!((vbits >> b) & 1) || L::empty(fw[b])) continue;
      uint32_t n = 0;
      if (L::match(fw[b], tag[b])) {
        hit1[b] = L::row1(fw[b]);
        n = 1;
      }
      if constexpr (L::CHAINED) {
        if (L::chain(fw[b])) {
          auto sl = layout.reindex(tag[b]);
          while (true) {
            sl = layout.next(sl);
            Word w = layout.load(sl);
            if (L::empty(w)) break;
            if (L::match(w, tag[b])) {
              if (n == 0) hit1[b] = L::row1(w);
              ++n;
            }
            if (!L::chain(w)) break;  // chain ends here
          }
        }
      }
      hit |= (uint32_t)(n != 0) << b;
      multi |= (uint32_t)(n > 1) << b;
      nm += n;
    }
    if (!FILL) {
      count_local += nm;
      continue;
    }
    uint32_t incl = wave_prefix_incl(nm);
    uint32_t total = __shfl(incl, WAVE - 1, WAVE);
    uint64_t wave_base = 0;
    if (lane == WAVE - 1 && total)
      wave_base = atomicAdd((unsigned long long*)counter,
                            (unsigned long long)total);
    wave_base = __shfl(wave_base, WAVE - 1, WAVE);
    int64_t pos = (int64_t)(wave_base + incl - nm);
    if (hit) {
#pragma unroll
      for (int b = 0; b < PPIPE; ++b) {
        if (!((hit >> b) & 1)) continue;
        int64_t prow = base + b;
        auto emit = [&](uint32_t r1) {
          if (pos < out_capacity) {
            out_build[pos] = (int32_t)(r1 - 1);
            out_probe[pos] = prow;
          }
          if (build_matched) build_matched[r1 - 1] = 1;
          ++pos;
        };
        if constexpr (L::CHAINED) {
          if (idxmap) prow = (int64_t)idxmap[base + b];
          if ((multi >> b) & 1) {
            // several matches: the first slot is not empty, walk it all again
            if (L::match(fw[b], tag[b])) emit(L::row1(fw[b]));
            if (L::chain(fw[b])) {
              auto sl = layout.reindex(tag[b]);
              while (true) {
                sl = layout.next(sl);
                Word w = layout.load(sl);
                if (L::empty(w)) break;
                if (L::match(w, tag[b])) emit(L::row1(w));
                if (!L::chain(w)) break;
              }
            }
            continue;
          }
        }
        emit(hit1[b]);
      }
    }
  }
  if (!FILL) {
    count_local = wave_sum(count_local);
    if (lane == 0 && count_local)
      atomicAdd((unsigned long long*)counter, (unsigned long long)count_local);
  }
}

// The one fill x validity ladder. Count mode passes null outputs.
template <typename L, typename K, int PPIPE>
void launch_probe(const K* probe, const uint8_t* pvalid, int64_t nprobe,
                  L layout, uint64_t* counter, int32_t* out_build,
                  int64_t* out_probe, int64_t out_capacity,
                  uint8_t* build_matched, int32_t fill, const int32_t* idxmap,
                  hipStream_t stream) {
  auto kernel =
      fill ? (pvalid ? join_probe_kernel_t<L, K, true, true, PPIPE>
                     : join_probe_kernel_t<L, K, true, false, PPIPE>)
           : (pvalid ? join_probe_kernel_t<L, K, false, true, PPIPE>
                     : join_probe_kernel_t<L, K, false, false, PPIPE>);
  if (!fill) {
    out_build = nullptr;
    out_probe = nullptr;
    out_capacity = 0;
    build_matched = nullptr;
    idxmap = nullptr;
  }
  kernel<<<grid_1d((nprobe + PPIPE - 1) / PPIPE), DEFAULT_BLOCK, 0, stream>>>(
      probe, pvalid, nprobe, layout, counter, out_build, out_probe,
      out_capacity, build_matched, idxmap);
}

}  // namespace srj
