// The join fast path's probe: one software-pipelined kernel over every table
// layout (join_fast.hip has the layouts and their build kernels).
//
// A workgroup takes a tile of BLOCK * PPIPE probe rows per iteration, PPIPE
// rows per lane:
//  * chained layouts give a lane PPIPE consecutive rows: one validity byte
//    per 8 rows gives the batch's live bits and the tail is clipped;
//    an unchained layout (at most one match per row) interleaves the rows of
//    a tile instead, row = tile base + b * BLOCK + thread, so that every key
//    load and every store instruction of a wave covers one contiguous run;
//  * a key that can never be in the table is masked out;
//  * keys, then slot indices, then ALL first-slot loads issue back to back
//    with nothing dependent between them — PPIPE outstanding random loads
//    per lane are the memory-level parallelism this kernel lives on;
//  * resolve counts each row's matches and carries the FIRST match's build
//    row in a register, so the (overwhelmingly common) exactly-one-match row
//    emits without walking its chain again;
//  * FILL reserves output space with one atomicAdd per workgroup and tile:
//    wave totals go through LDS, wave 0 scans them, adds their sum to the
//    counter and hands every wave its base (two barriers per tile), then
//    plain stores; only a row with several matches rescans its chain,
//    cache-warm. The interleaved mapping numbers its pairs b-major, so each
//    store instruction writes one contiguous run of out_build and out_probe.
//    A layout with WG_APPEND = false reserves per wave and batch instead, with
//    no barrier;
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
// What a probe emits is a compile-time mode, ProbeEmit. INNER is all of the
// above. The other two sit under `if constexpr`, so the INNER kernels are
// the code they were without them:
//  * OUTER (count and FILL): the left outer join. A row of [0, nprobe) that
//    resolve leaves without a match (null key, key that cannot be in the
//    table, or no match) becomes one pair of its own: its `hit` bit is set,
//    it counts 1 and its first-match register stays 0, so emit stores build
//    index 0 - 1 = -1 for it. emit leaves build_matched alone for such a
//    pair: there is no build row -1. The counter receives matching pairs
//    plus unmatched probe rows; reservation and capacity rules are INNER's.
//    idxmap is not supported (pass null).
//  * FLAG: one byte per probe row, probe_hit[row] = has_match ^ anti, and
//    nothing else: no counter, no LDS, no barrier, no atomic, no output
//    pairs, no build_matched. A chain walk ends at the first match. A null or
//    dead key has has_match = 0. probe_hit is 8-byte aligned and has
//    (nprobe + 15) / 16 * 16 bytes; every byte below nprobe is written, bytes
//    from nprobe up to the next multiple of 8 may be (with 0), nothing
//    beyond. A chained layout stores a lane's 8 consecutive flags as one
//    8-byte word at probe_hit + base, base a multiple of 8 (hence the
//    alignment rule), the interleaved layout one byte per b, a contiguous
//    run per wave.
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
//                 interleaved rows, and next, reindex and chain are not needed
//   WG_APPEND     one reservation per workgroup and tile (see above)
//   NT_OUT        optional; true: out_build and out_probe stores are nontemporal
#pragma once
#include <type_traits>

#include "srj_common.hpp"

namespace srj {

// what a probe emits (see above); the values are the entry points' `mode`
enum class ProbeEmit : int32_t { INNER = 0, OUTER = 1, FLAG = 2 };

// bit b of an 8-bit mask to byte b of a word: 8 flag bytes, one store
__device__ inline uint64_t bits_to_bytes(uint32_t m) {
  uint32_t lo = (m & 1u) | (m & 2u) << 7 | (m & 4u) << 14 | (m & 8u) << 21;
  m >>= 4;
  uint32_t hi = (m & 1u) | (m & 2u) << 7 | (m & 4u) << 14 | (m & 8u) << 21;
  return (uint64_t)hi << 32 | lo;
}

// A layout that declares NT_OUT = true has its pairs stored nontemporal: they
// are written once and never read by the kernel.
template <typename L, typename = void>
struct nt_out : std::false_type {};
template <typename L>
struct nt_out<L, std::enable_if_t<L::NT_OUT>> : std::true_type {};

template <typename L, typename K, bool FILL, bool HAS_VALID, int PPIPE,
          int BLOCK, ProbeEmit EMIT = ProbeEmit::INNER>
__global__ void __launch_bounds__(BLOCK, (PPIPE == 8 && !L::CHAINED) ? 8 : 1)
join_probe_kernel_t(const K* __restrict__ probe,
                    const uint8_t* __restrict__ pvalid, int64_t nprobe,
                    L layout, uint64_t* __restrict__ counter,
                    int32_t* __restrict__ out_build,
                    int64_t* __restrict__ out_probe, int64_t out_capacity,
                    uint8_t* __restrict__ build_matched,
                    const int32_t* __restrict__ idxmap,
                    uint8_t* __restrict__ probe_hit, uint32_t anti) {
  static_assert(PPIPE == 8 || PPIPE == 16, "validity bytes per batch");
  static_assert(L::WG_APPEND || L::CHAINED, "b-major needs the LDS table");
  static_assert(EMIT != ProbeEmit::FLAG || !FILL, "FLAG has no count or fill");
  constexpr bool OUTER = EMIT == ProbeEmit::OUTER;
  constexpr bool FLAG = EMIT == ProbeEmit::FLAG;
  using Tag = typename L::Tag;
  using Word = typename L::Word;
  constexpr bool ROWMAJOR = !L::CHAINED;
  constexpr int NW = BLOCK / WAVE;
  // reservation entries of a tile, in output order
  constexpr int NE = ROWMAJOR ? NW * PPIPE : NW;
  constexpr int EPL = (NE + WAVE - 1) / WAVE;  // entries per lane of wave 0
  constexpr int64_t TILE = (int64_t)BLOCK * PPIPE;
  constexpr int64_t STEP = ROWMAJOR ? BLOCK : 1;  // row = base + b * STEP
  __shared__ uint32_t cnt[NE];
  __shared__ uint64_t offs[NE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  uint64_t count_local = 0;
  const int64_t ntiles = (nprobe + TILE - 1) / TILE;
  // uniform per workgroup: every thread passes the same barriers
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t tbase = tile * TILE;
    const int64_t base = tbase + (int64_t)threadIdx.x * (ROWMAJOR ? 1 : PPIPE);
    uint32_t vbits = (1u << PPIPE) - 1u;
    // OUTER, FLAG: rows inside [0, nprobe), which vbits folds into "valid"
    [[maybe_unused]] uint32_t inb = (1u << PPIPE) - 1u;
    K k[PPIPE];
    if (ROWMAJOR) {
      uint32_t vb[PPIPE];
      if (tbase + TILE <= nprobe) {
        // a whole tile: one uniform base per b, the thread is the offset
#pragma unroll
        for (int b = 0; b < PPIPE; ++b) {
          k[b] = (probe + tbase + b * STEP)[threadIdx.x];
          vb[b] = HAS_VALID ? (uint32_t)(pvalid + ((tbase + b * STEP) >> 3))
                                      [threadIdx.x >> 3] >> (threadIdx.x & 7)
                            : 1u;
        }
      } else {
#pragma unroll
        for (int b = 0; b < PPIPE; ++b) {
          int64_t row = base + b * STEP;
          int64_t crow = row < nprobe ? row : 0;  // clamped, unconditional
          k[b] = probe[crow];
          vb[b] = HAS_VALID ? (uint32_t)pvalid[crow >> 3] >> (crow & 7) : 1u;
          if (row >= nprobe) vb[b] = 0;
          if constexpr (OUTER || FLAG)
            if (row >= nprobe) inb &= ~(1u << b);
        }
      }
      vbits = 0;
#pragma unroll
      for (int b = 0; b < PPIPE; ++b) vbits |= (vb[b] & 1u) << b;
    } else {
      if (HAS_VALID && base < nprobe) {
        vbits = pvalid[base >> 3];
        // the second byte of a 16-row batch may lie past the mask's last byte
        if (PPIPE == 16 && base + 8 < nprobe)
          vbits |= (uint32_t)pvalid[(base >> 3) + 1] << 8;
      }
      if (base + PPIPE > nprobe) {
        int64_t tail = nprobe - base;
        vbits &= (uint32_t)((1u << (tail < 0 ? 0 : tail)) - 1u);
        if constexpr (OUTER || FLAG)
          inb = (uint32_t)((1u << (tail < 0 ? 0 : tail)) - 1u);
      }
#pragma unroll
      for (int b = 0; b < PPIPE; ++b) {
        int64_t row = base + b;
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
    if constexpr (FLAG) {
      // has_match alone: a chain walk ends at the first match
      uint32_t hit = 0;
#pragma unroll
      for (int b = 0; b < PPIPE; ++b) {
        if (!((vbits >> b) & 1) || L::empty(fw[b])) continue;
        bool m = L::match(fw[b], tag[b]);
        if constexpr (L::CHAINED) {
          if (!m && L::chain(fw[b])) {
            auto sl = layout.reindex(tag[b]);
            while (true) {
              sl = layout.next(sl);
              Word w = layout.load(sl);
              if (L::empty(w)) break;
              m = L::match(w, tag[b]);
              if (m || !L::chain(w)) break;
            }
          }
        }
        hit |= (uint32_t)m << b;
      }
      // rows past nprobe get 0 whatever anti is
      const uint32_t flags = (hit ^ (anti ? ~0u : 0u)) & inb;
      if constexpr (ROWMAJOR) {
#pragma unroll
        for (int b = 0; b < PPIPE; ++b)
          if ((inb >> b) & 1)
            probe_hit[base + b * STEP] = (uint8_t)((flags >> b) & 1u);
      } else {
        // probe_hit is 8-byte aligned, base is a multiple of 8 and the
        // buffer is padded to 16: a word that starts below nprobe is aligned
        // and ends inside the buffer
#pragma unroll
        for (int w = 0; w < PPIPE / 8; ++w)
          if (base + 8 * w < nprobe)
            *reinterpret_cast<uint64_t*>(probe_hit + base + 8 * w) =
                bits_to_bytes((flags >> (8 * w)) & 0xffu);
      }
      continue;
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
    if constexpr (OUTER) {
      // an unmatched row inside is a pair of its own; its hit1 is still 0
      const uint32_t lone = inb & ~hit;
      hit |= lone;
      nm += (uint32_t)__popc(lone);
    }
    if (!FILL) {
      count_local += nm;
      continue;
    }
    // ROWMAJOR: per b, the hits of this wave's lower lanes, a byte each (the
    // ballots themselves must not stay in scalar registers over the barriers)
    uint32_t below[ROWMAJOR ? PPIPE / 4 : 1] = {};
    uint32_t incl = 0;      // lane-major: inclusive wave scan of nm
    uint64_t wave_base = 0;  // lane-major: first output position of the wave
    if constexpr (ROWMAJOR) {
      uint32_t mine = 0;
#pragma unroll
      for (int b = 0; b < PPIPE; ++b) {
        uint64_t m = __ballot((hit >> b) & 1);
        below[b / 4] |= __builtin_amdgcn_mbcnt_hi(
                            (uint32_t)(m >> 32),
                            __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))
                        << (8 * (b % 4));
        if (lane == b) mine = (uint32_t)__popcll(m);
      }
      // one entry per (b, wave), b-major
      if (lane < PPIPE) cnt[lane * NW + wave] = mine;
    } else {
      incl = wave_prefix_incl(nm);
      if (L::WG_APPEND && lane == WAVE - 1) cnt[wave] = incl;
    }
    if constexpr (L::WG_APPEND) {
      __syncthreads();
      if (wave == 0) {
        uint32_t c[EPL], sum = 0;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          int i = lane * EPL + e;
          c[e] = i < NE ? cnt[i] : 0u;
          sum += c[e];
        }
        uint32_t sincl = wave_prefix_incl(sum);
        uint32_t total = __shfl(sincl, WAVE - 1, WAVE);
        uint64_t run = 0;
        if (lane == WAVE - 1 && total)
          run = atomicAdd((unsigned long long*)counter,
                          (unsigned long long)total);
        run = __shfl(run, WAVE - 1, WAVE) + sincl - sum;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          int i = lane * EPL + e;
          if (i < NE) offs[i] = run;
          run += c[e];
        }
      }
      // offs is rewritten only behind the next tile's first barrier, cnt only
      // behind this one: two barriers per tile are enough
      __syncthreads();
      if (!ROWMAJOR) wave_base = offs[wave];
    } else {
      uint32_t total = __shfl(incl, WAVE - 1, WAVE);
      if (lane == WAVE - 1 && total)
        wave_base = atomicAdd((unsigned long long*)counter,
                              (unsigned long long)total);
      wave_base = __shfl(wave_base, WAVE - 1, WAVE);
    }
    if (hit) {
      int64_t pos = (int64_t)(wave_base + incl - nm);
#pragma unroll
      for (int b = 0; b < PPIPE; ++b) {
        if (!((hit >> b) & 1)) continue;
        int64_t prow = base + b * STEP;
        if constexpr (ROWMAJOR)
          pos = (int64_t)offs[b * NW + wave] +
                ((below[b / 4] >> (8 * (b % 4))) & 0xffu);
        auto emit = [&](uint32_t r1) {
          if (pos < out_capacity) {
            if constexpr (nt_out<L>::value) {
              __builtin_nontemporal_store((int32_t)(r1 - 1), &out_build[pos]);
              __builtin_nontemporal_store(prow, &out_probe[pos]);
            } else {
              out_build[pos] = (int32_t)(r1 - 1);
              out_probe[pos] = prow;
            }
          }
          // OUTER: r1 == 0 is an unmatched probe row, build index -1
          if (build_matched && (!OUTER || r1)) build_matched[r1 - 1] = 1;
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
  if (!FILL && !FLAG) {
    count_local = wave_sum(count_local);
    if (lane == 0 && count_local)
      atomicAdd((unsigned long long*)counter, (unsigned long long)count_local);
  }
}

// The one emit x fill x validity ladder. Count mode passes null outputs;
// FLAG writes probe_hit alone and ignores fill.
template <typename L, typename K, int PPIPE, int BLOCK>
void launch_probe(const K* probe, const uint8_t* pvalid, int64_t nprobe,
                  L layout, uint64_t* counter, int32_t* out_build,
                  int64_t* out_probe, int64_t out_capacity,
                  uint8_t* build_matched, int32_t fill, const int32_t* idxmap,
                  hipStream_t stream, ProbeEmit emit = ProbeEmit::INNER,
                  uint8_t* probe_hit = nullptr, int32_t anti = 0) {
  constexpr ProbeEmit I = ProbeEmit::INNER, O = ProbeEmit::OUTER,
                      F = ProbeEmit::FLAG;
  auto pick = [&](auto with_valid) {
    constexpr bool V = decltype(with_valid)::value;
    if (emit == F) return join_probe_kernel_t<L, K, false, V, PPIPE, BLOCK, F>;
    if (emit == O)
      return fill ? join_probe_kernel_t<L, K, true, V, PPIPE, BLOCK, O>
                  : join_probe_kernel_t<L, K, false, V, PPIPE, BLOCK, O>;
    return fill ? join_probe_kernel_t<L, K, true, V, PPIPE, BLOCK, I>
                : join_probe_kernel_t<L, K, false, V, PPIPE, BLOCK, I>;
  };
  auto kernel = pvalid ? pick(std::true_type{}) : pick(std::false_type{});
  if (!fill || emit == F) {
    out_build = nullptr;
    out_probe = nullptr;
    out_capacity = 0;
    build_matched = nullptr;
    idxmap = nullptr;
  }
  if (emit != I) idxmap = nullptr;
  if (emit != F) probe_hit = nullptr;
  // one tile of BLOCK * PPIPE rows per workgroup and iteration; the cap
  // keeps MAX_GRID * DEFAULT_BLOCK threads whatever the workgroup size
  kernel<<<grid_1d((nprobe + PPIPE - 1) / PPIPE, BLOCK,
                   MAX_GRID * DEFAULT_BLOCK / BLOCK),
           BLOCK, 0, stream>>>(probe, pvalid, nprobe, layout, counter,
                               out_build, out_probe, out_capacity,
                               build_matched, idxmap, probe_hit,
                               (uint32_t)(anti != 0));
}

}  // namespace srj
