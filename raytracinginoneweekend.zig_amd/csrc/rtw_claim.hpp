// rtw_claim.hpp — guided claims on the megakernel's unit queue (rtw_trace.hip take_units, the primary-first
// loop): a wave claims K consecutive 64-unit batches with ONE atomic on the launch's counter and keeps the
// ones it has not fetched yet as its reserve.  Consecutive batches are one tile's successive chunks (the chunk
// is the fastest index of a batch, rtw_device.hpp dealt_unit, in both unit orders), so the tile's beam pass —
// its sphere mask and its "no camera ray can hit a sphere" verdict, which do not depend on the chunk — is
// made once for them.
//
// K is larger than 1 only in a run of proven-empty batches, and at most the run's length so far (claim_k):
// batches finished without tracing cost little more than the atomic, and they come in runs (the sky's tiles
// lead the queue in image order), while a traced batch is dozens of wave-iterations, and traced batches
// waiting in reserves made every traced frame slower, by 4 % (K = 2) to 80 % (K = 8) when every claim was
// guided: profiles/r19/README.md.  A reserve therefore holds traced batches only where a run ends, fewer
// than the run was long.  Within a run K is guided self-scheduling's: the batches left behind the last queue head the wave saw, divided among
// kClaimDiv x the launch's waves, between 1 and kClaimMax; it falls to 1 while every wave still has
// kClaimDiv claims to come, so the launch's tail is dealt batch by batch as before.
//
// Invariants (tests/native/claim_check.cpp simulates waves against one counter):
//  * every unit of the queue is fetched exactly once: claims are disjoint ranges of one atomic counter, and a
//    reserve is fetched first to last, each batch once;
//  * a wave fetches its batches in ascending queue order: it claims only with an empty reserve, the counter
//    only grows, and reserve_next hands the reserve out from its low end;
//  * a wave's claim reaches at most kClaimMax batches past the queue's end, and a fetched batch at or past
//    the end empties the reserve (every later one lies past the end too).
// Host and device code; no HIP types.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RTWC_HD __host__ __device__ __forceinline__
#else
#define RTWC_HD inline
#endif

namespace rtwc {

constexpr uint32_t kClaimBatch = 64;  // units per batch (rtw_internal.hpp kBatch)
#ifndef RTW_CLAIM_MAX
#define RTW_CLAIM_MAX 8
#endif
#ifndef RTW_CLAIM_DIV
#define RTW_CLAIM_DIV 2
#endif
constexpr uint32_t kClaimMax = RTW_CLAIM_MAX;  // Kmax and c: the A/B of {2, 4, 8} x {2, 4}, profiles/r19/README.md
constexpr uint32_t kClaimDiv = RTW_CLAIM_DIV;

// A wave's reserve: the claimed whole batches [next, end) it has not fetched (queue indices, multiples of 64).
// `end` outlives the reserve: it is the queue head right after the wave's last claim, the head guided_k uses.
struct Reserve {
  uint32_t next = 0, end = 0;
};

// Batches of the next claim.  head: the last queue head the wave saw (0 before its first claim); div_waves:
// kClaimDiv x the launch's waves, 0 = claims of one batch.  floor(left / div_waves) clamped to [1, kClaimMax],
// as compares: no division in the kernel.
RTWC_HD uint32_t guided_k(uint32_t head, uint32_t total_units, uint32_t div_waves) {
  if (div_waves == 0u) return 1u;
  const uint32_t left = head < total_units ? (total_units - head) / kClaimBatch : 0u;
  uint32_t k = 1u;
  for (uint32_t j = 2u; j <= kClaimMax; ++j) k += left >= j * div_waves ? 1u : 0u;
  return k;
}

// The reserve after a claim of k batches that the counter answered with `base`; its first batch is fetched
// at once (after_fetch), the others wait.
RTWC_HD Reserve after_claim(uint32_t base, uint32_t k) { return {base, base + k * kClaimBatch}; }

// Whether the reserve holds a batch.
RTWC_HD bool reserve_has(const Reserve& r) { return r.next < r.end; }

// The reserve after its lowest batch `base` (== r.next) was fetched: the next one up, or nothing once `base`
// lies at or past the queue's end.
RTWC_HD Reserve after_fetch(const Reserve& r, uint32_t base, uint32_t total_units) {
  return {base < total_units ? base + kClaimBatch : r.end, r.end};
}

// The wave's last beam pass as one word: its tile (< 2^24: a frame has at most 2^24 pixels) and, in bit 31,
// its verdict "no camera ray of the tile can hit a sphere".  kNoPass: none yet; it names no tile.
constexpr uint32_t kNoPass = 0x7FFFFFFFu;
RTWC_HD uint32_t pass_word(uint32_t tile, uint32_t empty) { return (tile & 0x7FFFFFFFu) | (empty << 31); }
RTWC_HD uint32_t pass_empty(uint32_t word) { return word >> 31; }
// The wave's run of proven-empty batches after it fetched one more batch of the queue (counted up to kClaimMax).
RTWC_HD uint32_t run_after(uint32_t run, uint32_t empty) { return empty ? (run < kClaimMax ? run + 1u : run) : 0u; }
// Batches of the next claim: the run's length so far, at least one, at most guided_k.
RTWC_HD uint32_t claim_k(uint32_t run, uint32_t head, uint32_t total_units, uint32_t div_waves) {
  if (run < 2u) return 1u;
  const uint32_t g = guided_k(head, total_units, div_waves);
  return run < g ? run : g;
}
// Whether a batch of tile `tile` may reuse the pass `word`: one batch is one (tile, chunk) in both unit orders,
// and neither the mask nor the verdict depends on the chunk.
RTWC_HD bool same_tile(uint32_t tile, uint32_t word) { return tile == (word & 0x7FFFFFFFu); }

}  // namespace rtwc
