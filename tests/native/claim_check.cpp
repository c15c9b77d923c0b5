// claim_check.cpp — host check of the megakernel's guided claims (csrc/rtw_claim.hpp): W waves fetch 64-unit
// batches from one counter exactly as rtw_trace.hip take_units does — from the wave's reserve when it holds
// a batch, else by one claim of claim_k batches — in seeded random interleavings, for both unit orders and
// for queue lengths around multiples of kClaimMax batches.  Checked per simulation:
//   * every batch of the queue is fetched exactly once, none twice, none past the end by two waves;
//   * each wave's batches ascend;
//   * no wave claims more than kClaimMax x 64 units at or past the queue's end (it stops at its first batch
//     there, its reserve emptied), so the counter ends within waves x kClaimMax x 64 of the queue's length;
//   * guided_k is floor(batches left behind the head / div_waves) clamped to [1, kClaimMax] (by division
//     here, by compares there), so it is 1 once fewer than 2 x div_waves batches are left;
//   * a claim is no larger than the wave's run of proven-empty batches so far (one batch after a traced
//     one), and with div_waves = 0 every claim is one batch;
//   * a batch reuses the wave's last beam pass only for the pass's own tile, with the pass's verdict, and
//     the passes made are at most the claims plus the tile changes along the queue.
// Prints "sims N checks C violations V"; exit status 1 with violations.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "rtw_claim.hpp"

namespace {

uint64_t checks = 0, violations = 0, all_big_claims = 0;
void check(bool ok, const char* what, uint32_t a = 0, uint32_t b = 0) {
  ++checks;
  if (!ok) {
    if (++violations <= 20) fprintf(stderr, "violation: %s (%u, %u)\n", what, a, b);
  }
}

struct Wave {
  rtwc::Reserve r;
  uint32_t pass = rtwc::kNoPass;
  bool live = true, have_last = false;
  uint32_t run = 0, true_run = 0;  // consecutive proven-empty batches fetched: as the header counts, and recounted
  uint32_t last = 0, over = 0;  // over: units it claimed at or past the queue's end
};

// the tile of queue batch `base` (rtw_device.hpp dealt_unit, rtw_trace.hip decode_batch)
uint32_t tile_of(uint32_t base, uint32_t total, uint32_t nc, uint32_t order) {
  const uint32_t dealt = (order ? total - 1u - base : base) & ~63u;
  return (dealt >> 6) / nc;
}
// a verdict per tile the simulation can recompute
uint32_t empty_of(uint32_t tile) { return (tile * 2654435761u >> 13) & 1u; }

void simulate(uint32_t n_waves, uint32_t n_batches, uint32_t nc, uint32_t order, uint32_t div_waves, uint32_t seed) {
  const uint32_t total = n_batches * rtwc::kClaimBatch;
  std::mt19937 rng(seed);
  std::vector<Wave> w(n_waves);
  std::vector<uint32_t> taken(n_batches, 0), live;
  for (uint32_t i = 0; i < n_waves; ++i) live.push_back(i);
  uint32_t counter = 0;
  uint64_t claims = 0, passes = 0, big_claims = 0;
  while (!live.empty()) {
    const size_t pick = rng() % live.size();
    Wave& v = w[live[pick]];
    // one fetch, as take_units makes it
    if (!rtwc::reserve_has(v.r)) {
      const uint32_t head = v.r.end;
      const uint32_t k = div_waves ? rtwc::claim_k(v.run, head, total, div_waves) : 1u;
      const uint32_t left = head < total ? (total - head) / rtwc::kClaimBatch : 0u;
      uint32_t want = div_waves ? left / div_waves : 1u;
      want = want < 1u ? 1u : (want > rtwc::kClaimMax ? rtwc::kClaimMax : want);
      check(rtwc::guided_k(head, total, div_waves) == want, "guided_k is the clamped quotient", k, want);
      check(v.run == (v.true_run < rtwc::kClaimMax ? v.true_run : rtwc::kClaimMax), "the run is counted", v.run, v.true_run);
      const uint32_t by_run = v.true_run < 1u ? 1u : v.true_run;
      check(k == (by_run < want ? by_run : want), "a claim is at most the run of proven-empty batches so far", k, want);
      if (k > 1u) ++big_claims;
      if (div_waves && left < 2u * div_waves) check(k == 1u, "K is 1 near the queue's end", k, left);
      const uint32_t base = counter;
      counter += k * rtwc::kClaimBatch;
      v.r = rtwc::after_claim(base, k);
      check(v.r.end - base <= rtwc::kClaimMax * rtwc::kClaimBatch, "a claim is at most kClaimMax batches", base, v.r.end);
      if (v.r.end > total) v.over += v.r.end - (base > total ? base : total);
      ++claims;
    }
    const uint32_t base = v.r.next;
    v.r = rtwc::after_fetch(v.r, base, total);
    check(base % rtwc::kClaimBatch == 0u, "a batch is 64-aligned", base);
    if (v.have_last) check(base > v.last, "a wave's batches ascend", v.last, base);
    v.have_last = true, v.last = base;
    if (base >= total) {  // its units are refused: the wave is done, and holds nothing more
      check(!rtwc::reserve_has(v.r), "a batch past the end empties the reserve", v.r.next, v.r.end);
      v.live = false;
      live[pick] = live.back();
      live.pop_back();
      continue;
    }
    ++taken[base / rtwc::kClaimBatch];
    // the beam pass, made or reused
    const uint32_t tile = tile_of(base, total, nc, order);
    v.run = rtwc::run_after(v.run, empty_of(tile));
    v.true_run = empty_of(tile) ? v.true_run + 1u : 0u;
    if (div_waves != 0u && rtwc::same_tile(tile, v.pass)) {
      check(rtwc::pass_empty(v.pass) == empty_of(tile), "a reused verdict is the tile's", tile);
    } else {
      v.pass = rtwc::pass_word(tile, empty_of(tile));
      check(rtwc::same_tile(tile, v.pass) && rtwc::pass_empty(v.pass) == empty_of(tile), "pass word round trip", tile);
      ++passes;
    }
  }
  for (uint32_t b = 0; b < n_batches; ++b) check(taken[b] == 1u, "every batch is fetched exactly once", b, taken[b]);
  for (const Wave& v : w)
    check(v.over <= rtwc::kClaimMax * rtwc::kClaimBatch, "overshoot within kClaimMax x 64 units", v.over, total);
  check(counter <= total + n_waves * rtwc::kClaimMax * rtwc::kClaimBatch, "the counter's end", counter, total);
  const uint32_t n_tiles = (n_batches + nc - 1u) / nc;
  check(passes <= claims + (n_tiles ? n_tiles - 1u : 0u), "passes <= claims + tile changes", (uint32_t)passes, (uint32_t)claims);
  if (div_waves == 0u) check(claims == (uint64_t)n_batches + n_waves, "claims of one batch", (uint32_t)claims, n_batches);
  all_big_claims += big_claims;
}

}  // namespace

int main() {
  uint64_t sims = 0;
  check(rtwc::kNoPass != 0u && !rtwc::same_tile(0u, rtwc::kNoPass) && !rtwc::same_tile((1u << 24) - 1u, rtwc::kNoPass),
        "kNoPass names no tile");
  const uint32_t km = rtwc::kClaimMax;
  for (uint32_t n_waves : {1u, 3u, 16u, 64u})
    for (uint32_t mult : {0u, 1u, 2u, 7u, 40u, 300u})
      for (int d = -2; d <= 2; ++d) {
        const int nb = (int)(mult * km * n_waves) + d;
        if (nb < 0) continue;
        for (uint32_t nc : {1u, 2u, 5u, 7u, 25u})
          for (uint32_t order : {0u, 1u})
            for (uint32_t div : {0u, rtwc::kClaimDiv * n_waves})
              for (uint32_t seed = 1; seed <= 3; ++seed) {
                simulate(n_waves, (uint32_t)nb, nc, order, div, seed * 7919u + (uint32_t)nb);
                ++sims;
              }
      }
  // queue lengths near the 32-bit limit of the plan (rtw_plan.cpp: units <= 2^31 - 1): the arithmetic does not wrap
  {
    const uint32_t total = 0x7FFFFFC0u, waves = 4096u, div = rtwc::kClaimDiv * waves;
    check(rtwc::guided_k(0u, total, div) == km, "K at the head of the longest queue");
    check(rtwc::guided_k(total - 64u, total, div) == 1u, "K at its end");
    check(rtwc::guided_k(total + waves * km * 64u, total, div) == 1u, "K past its end");
    const rtwc::Reserve r = rtwc::after_claim(total - 64u, km);
    check(r.end == total - 64u + km * 64u && r.end > r.next, "a claim across the end does not wrap", r.next, r.end);
    check(total + waves * km * 64u > total, "every wave's overshoot fits 32 bits");
  }
  if (km > 1u) check(all_big_claims > 10000u, "empty runs of long queues are claimed several batches at a time", (uint32_t)all_big_claims);
  printf("sims %llu checks %llu violations %llu\n", (unsigned long long)sims, (unsigned long long)checks,
         (unsigned long long)violations);
  return violations ? 1 : 0;
}
