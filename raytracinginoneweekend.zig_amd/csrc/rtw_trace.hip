// rtw_trace.hip — CDNA4 (gfx950) megakernel for the RTIOW cover-scene render
// loop: the reference's main.zig:378-402 loop + rayColor (main.zig:103-122)
// + HittableList/Sphere/MovingSphere.hit (hittable.zig:95-244) +
// Lambertian/Metal/Dielectric.scatter (material.zig:44-121) + Solid/Checker
// textures (texture.zig:46-83), re-designed for 64-wide wavefronts.
//
// Design (DESIGN.md has the full rationale):
//  * Work unit = (pixel, chunk of `chunk` samples).  Units are dealt from ONE
//    device counter in batches of 64 per wave (one atomic per 64 units); a
//    lane that finishes its unit takes the next one from the wave's batch at
//    once ("lane-level regeneration"), so lanes never wait for the slowest
//    path of the wave and the end-of-launch drain is one chunk long.
//  * Per lane, one loop iteration = [take a unit] -> [start a sample: the
//    sample's counter-RNG block, camera ray] -> [one bounce segment].  Paths
//    of different length share the wave without padding to the longest.  The
//    loop rotates the iteration so that the lens-disk points of the new
//    samples and the unit-ball points of the hits come from ONE cooperative
//    rejection pass (the rotated loop below).  The f64 kernel of a full frame
//    goes one step further (TraceCfg::kPrimaryFirst, the primary-first loop):
//    a lane that starts a sample resolves its camera ray itself — the wide
//    spheres, then the exact tests of the few spheres in the mask of its
//    tile (rtw_beam.hpp, made once per 64-unit batch in take_units) — and
//    shades that hit in the same iteration, so a sample whose camera ray hits
//    takes one wave-iteration less; only secondary rays go through the
//    wave-uniform pretest.
//  * The closest-hit loop over the sphere list is wave-UNIFORM: every lane
//    tests sphere k at the same time, so sphere k's record is fetched with
//    scalar loads (s_load, SGPR operands of the VALU ops): zero VGPRs and zero
//    LDS traffic for the hottest data.  The per-lane lookups that follow (the
//    winning sphere, its material) index LDS copies of the tables.
//  * Arithmetic follows the reference operation by operation (compiled with
//    -ffp-contract=off): precision 0 is the reference's f64; precision 1 is
//    f32 with wide (radius >= 100) spheres solved in f64 and convex self-skip.
//  * Per-chunk sums (f64) go to HBM; a second kernel adds chunks in order and
//    quantises exactly like main.zig:395-400.
// The oracle's tierb_core.h is the written contract this file implements.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rtw_claim.hpp"
#include "rtw_device.hpp"

// (Round 4) The lane's state flags (have_unit, have_ray, done, shading) as bits of one
// u32 (rtw_device.hpp LaneFlag) instead of bools: as bools they were 64-bit
// lane masks in SGPRs for the whole loop, and at the 100-SGPR limit the loop
// spilled SGPRs to VGPR lanes and one 8-B pair to scratch.  Hot loop: 14 -> 6
// lane ops, 2 -> 1 scratch pairs; -1.4 % per configs[1] frame
// (profiles/r04/trace_lane_flags_ab.txt).

namespace rtwk {

// The kernel's configurations: one per precision and kind of launch (MASKED: a masked accumulator pass,
// DESIGN.md §13; else a frame or an unmasked pass).  Each line names the measurement that decided it; the
// arms that lost are DESIGN.md §6's table of retired variants.  In every configuration:
//  - the closest hit reads the scene fields from the kernel argument (SGPR budget; +0.8 % f64, +1.0 % f32,
//    profiles/r01/ab_defaults.txt);
//  - the rotated loop (+5.3 % f64, +4.1 % f32) with the sample's time draw and the dielectric's draw made in
//    its cooperative pass (+1.2 % f64; both profiles/r01/ab_defaults.txt);
//  - Schlick's r0^2 from the material table and, in f64, the fast exact sqrt (+0.4 % f64 together,
//    profiles/r01/ab_defaults.txt) and the clustered pretest (+5.4 %, profiles/r02/cluster_ab.txt);
//  - the lane's unit fields and f64 chunk sum in the wave's LDS home block (+0.6 % f64, +1.3 % f32,
//    profiles/r03/home_lds_ab.txt, home_lds_f32_ab.txt).
template <bool F32, bool MASKED>
struct TraceCfg {
  // Waves per SIMD the register allocator is asked for: 4 (128 VGPRs) in f64, 5 (96) in f32
  // (profiles/r01/ab_defaults.txt); the masked f32 pass 4, since at 96 the map's two loads spilled 32 B of
  // scratch against the unmasked kernel's 16.
  static constexpr int kWavesPerSimd = (F32 && !MASKED) ? 5 : 4;
  // The loop's argument fields re-read from the kernel argument where used, not held in SGPRs for the whole
  // kernel: f64 only (+0.6 %, profiles/r02/var1024_ab.txt).
  static constexpr bool kLoopArgsFromKernarg = !F32;
  // The primary-first loop, its new samples' lens-disk points from each lane's own rejection loop: f64 frames
  // (profiles/r11/README.md, bench_ab.txt); a masked pass keeps the rotated loop with the cooperative disk.
  static constexpr bool kPrimaryFirst = !F32 && !MASKED;
  // Bytes per wave after the scene tables (rtw_internal.hpp): the home block, then the primary masks.
  static constexpr size_t kHomeStride = kHomeLdsBytesPerWave + (kPrimaryFirst ? kPrimaryLdsBytesPerWave : 0);
  // Bytes per wave after those, in a launch with TraceArgs::tail_on: the tail block of the primary-first loop
  // (profiles/r15/README.md).
  static constexpr size_t kTailBytes = kPrimaryFirst ? kTailLdsBytesPerWave : 0;
  // The exact tests' "both roots behind" prefilter is rtw_selfskip.hpp's rule (closest_hit LEAVEPRE): the sphere a
  // secondary ray has just left ends its test there.  f64 frames: -1.26 % per configs[1] frame
  // (profiles/r25/README.md).  -DRTW_NO_SELFSKIP: the parent's prefilter, the measurement build of that A/B.
#ifdef RTW_NO_SELFSKIP
  static constexpr bool kLeavePre = false;
#else
  static constexpr bool kLeavePre = !F32 && !MASKED;
#endif
};

template <typename R, bool F32, int MODE, bool MASKED>
__global__ void __launch_bounds__(kTraceBlock, (TraceCfg<F32, MASKED>::kWavesPerSimd)) trace_kernel(TraceArgs<R> A) {
  using Cfg = TraceCfg<F32, MASKED>;
  constexpr bool STATS = MODE == 1;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const SceneView<R> S = A.sc;
  // LDS: per-wave coop_reject slots, then copies of the per-lane lookup
  // tables (winning sphere, its material).
  const LdsTables<R> T = stage_tables<R>(S, lds_raw);
  CoopSlots* slots = T.slots;

  const uint32_t lid = lane_id();
  // The lane's unit fields (pixel, chunk, sample end) and its f64 chunk sum
  // live in this wave's LDS home block (SoA, one entry per lane) instead of
  // 10 VGPRs held across the closest hit; they are touched only when a unit
  // starts or ends, a sample starts, or a path misses.
  // (Declared, then set: with the pointers initialised in place the counts kernel of f32 is allocated
  // otherwise, 5 instructions apart; profiles/r12/isa_identity.txt.)
  double* h_sum = nullptr;    // [3][64]
  uint32_t* h_u32 = nullptr;  // px[64], ly[64], c[64], s_end[64]
  {
    const size_t off = (size_t)(reinterpret_cast<unsigned char*>(T.cpos + kClusterSlots * S.n_clusters) - lds_raw);
    // (a launch with TraceArgs::tail_on: the wave's tail block follows its primary masks)
    const size_t stride = Cfg::kHomeStride + (Cfg::kTailBytes != 0 && A.tail_on ? Cfg::kTailBytes : 0);
    unsigned char* hb = lds_raw + ((off + 7) & ~(size_t)7) + (threadIdx.x >> 6) * stride;
    h_sum = reinterpret_cast<double*>(hb);
    h_u32 = reinterpret_cast<uint32_t*>(hb + 3 * 64 * 8);
    // (the primary masks are h_u32[256 ...]: right after it, the same address register with other offsets)
  }
  // Cfg::kLoopArgsFromKernarg: the loop's kernel-argument fields are re-read
  // where used (scalar loads through a laundered kernarg pointer) instead of
  // living in SGPRs for the whole kernel: the SGPR budget is the limit (spills
  // become v_readlane/v_writelane VALU instructions).
#define RTW_KA(f) (Cfg::kLoopArgsFromKernarg ? opaque(kargs<R>())->f : A.f)
  const R kInf = (R)__builtin_huge_val();

  Lane<R> L;
  L.px = L.ly = L.s = L.depth = 0;
  L.rs = 0;
  L.skip = -1;
  uint32_t lane_flags = 0u;  // (rtw_device.hpp LaneFlag)
  LaneFlag<1u> have_unit{lane_flags};
  LaneFlag<2u> have_ray{lane_flags};
  LaneFlag<4u> done{lane_flags};
  uint32_t qnext = 0, qend = 0;  // wave-uniform batch [qnext, qend)
  KStats st;
  if constexpr (MODE == 2) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st.t_last)::"memory");

  // MASKED: the dealt tile index counts the active tiles only, tile_list gives
  // the frame's tile, and a unit whose pixel's bit of the tile's mask is clear
  // is skipped as a padding unit is.
  // Cfg::kPrimaryFirst: the sphere mask of a unit batch's tile (wave-uniform; bit order of
  // SceneView::cvalid), in LDS, not in registers held across the loop: h_u32[kPm + 64 h + lid] = word h
  // of the mask of the lane's own batch, h_u32[kBm + 64 h + lid] = of the wave's current batch (a copy
  // per lane: every LDS address of the take is the lane's h_u32 address plus a constant).
  constexpr uint32_t kPm = 4 * 64, kBm = 6 * 64;
  uint32_t* const h_me = h_u32 + lid;
  constexpr bool PF = Cfg::kPrimaryFirst;
  // Cfg::kPrimaryFirst: the wave's claim words after the masks (wave-uniform, kClaimLdsBytesPerWave):
  // h_u32[kRs], [kRs + 1] = the reserve of claimed batches [next, end), [kRs + 2] = the tile of the wave's
  // last beam pass with its verdict, [kRs + 3], [kRs + 4] = that pass's mask words, [kRs + 5] = its run of
  // proven-empty batches (rtw_claim.hpp; take_units).
  // In LDS, not in registers held across the closest hit.
  constexpr uint32_t kRs = 8 * 64;
  // (made from the lane's own h_me where used, the lane index laundered: no address of them lives in a register
  // of the loop)
  auto claim_words = [&]() __attribute__((always_inline)) -> uint32_t* {
    uint32_t l = lid;
    asm volatile("" : "+v"(l));
    return h_me - l + kRs;
  };
  if constexpr (PF) {
    uint32_t* const cwd = claim_words();
    cwd[0] = 0u, cwd[1] = 0u, cwd[2] = rtwc::kNoPass, cwd[5] = 0u;
  }
  // Cfg::kPrimaryFirst: (tile x, tile y, chunk) of a newly fetched unit batch (wave-uniform).  A batch is 64
  // aligned units = one (tile, chunk): decoded once, for the tile's beam.
  // (nb_pad is never written.  The kernels were measured with a 64-bit word in this place; without it the
  // compiler numbers three VGPRs of the f64 kernels otherwise — the same instructions — and the library
  // would not be the one profiles/r11 measured: profiles/r12/isa_identity.txt.)
  uint32_t nb_tx = 0, nb_ty = 0, nb_c = 0;
  uint64_t nb_pad = 0;
  auto decode_batch = [&](uint32_t base, uint32_t& tx, uint32_t& ty, uint32_t& c, uint64_t& pad) {
    const uint32_t b64 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 6));
    const uint32_t nc = RTW_KA(n_chunks), txs = RTW_KA(tiles_x);
    const uint32_t tile = b64 / nc;
    c = b64 - tile * nc;
    ty = tile / txs;
    tx = tile - ty * txs;
  };
  // ---- take units for lanes that need one (wave-uniform control) ----
  // (always_inline: the primary-first kernel calls it from both of its loops, and out of line its captures
  // are in scratch memory)
  auto take_units = [&]() __attribute__((always_inline)) {
    const bool need = !have_unit && !done;
    const uint64_t needmask = __ballot(need);
    if (needmask) {
      const uint32_t n = (uint32_t)__popcll(needmask);
      const uint32_t rank = mbcnt64(needmask);
      const uint32_t rem = qend - qnext;
      uint32_t base2 = 0;
      uint32_t nb_bm0 = 0u, nb_bm1 = 0u;
      // (PF: a loop only over batches finished without tracing, TraceArgs::empty_on, below)
      // PF with TraceArgs::claim_waves (rtw_claim.hpp): the wave claims K batches with one atomic and fetches
      // the others from its reserve, and a batch of the tile of the wave's last beam pass reuses that pass.
      // The reserve and the last pass — its tile with its verdict, its mask words — are wave-uniform words of
      // the wave's LDS (h_u32[kRs ...]), read and written where used: nothing of them is held in a register
      // across the beam pass or the closest hit.  Ascending order: a claim is made only with an empty
      // reserve, the counter only grows, and the reserve is handed out from its low end; a batch at or past
      // the queue's end empties it (after_fetch), so one refused unit still means all later ones are refused.
      uint32_t nb_empty = 0u;
      if (n > rem) for (;;) {
        uint32_t b = 0;
        if constexpr (!PF) {
          if (lid == 0) b = atomicAdd(RTW_KA(counter), kBatch);
          base2 = __shfl(b, 0);
          break;
        } else {
          const uint32_t cw = RTW_KA(claim_waves);
          uint32_t* const cwd = claim_words();
          rtwc::Reserve rs;
          if (cw != 0u) rs.next = cwd[0], rs.end = cwd[1];
          if (!rtwc::reserve_has(rs)) {
            const uint32_t k = cw != 0u ? rtwc::claim_k(cwd[5], rs.end, RTW_KA(total_units), cw) : 1u;
            if (lid == 0) b = atomicAdd(RTW_KA(counter), k * kBatch);
            // (lane 0's value by a constant address: __shfl's lane arithmetic was held in a register)
            rs = rtwc::after_claim((uint32_t)__builtin_amdgcn_ds_bpermute(0, (int)b), k);
            if constexpr (STATS) {
              if (lid == 0) st.claims++;
            }
          }
          base2 = rs.next;
          if (cw != 0u) {
            rs = rtwc::after_fetch(rs, base2, RTW_KA(total_units));
            cwd[0] = rs.next, cwd[1] = rs.end;  // (every lane, the same words)
          }
          // (a dealt batch is a 64-aligned batch in every order)
          decode_batch(dealt_unit(base2, *opaque(kargs<R>())) & ~63u, nb_tx, nb_ty, nb_c, nb_pad);
          // The new batch's mask: which clustered slots can a camera ray of its
          // tile hit (rtw_beam.hpp)?  Lane j answers for slot j; every lane of
          // the wave is here (wave-uniform branch at the loop's top).  A batch
          // past the queue's end names no tile: its units are refused below.
          if (!RTW_KA(primary_on)) break;
          const auto* ka = opaque(kargs<R>());
          const uint32_t last = cwd[2];
          if (cw != 0u && rtwc::same_tile(nb_ty * ka->tiles_x + nb_tx, last)) {
            nb_bm0 = cwd[3], nb_bm1 = cwd[4];
            nb_empty = rtwc::pass_empty(last);
          } else {
            const double org[3] = {ka->origin[0], ka->origin[1], ka->origin[2]};
            const double llc[3] = {ka->llc[0], ka->llc[1], ka->llc[2]};
            const double hor[3] = {ka->horizontal[0], ka->horizontal[1], ka->horizontal[2]};
            const double ver[3] = {ka->vertical[0], ka->vertical[1], ka->vertical[2]};
            const double cu[3] = {ka->cu[0], ka->cu[1], ka->cu[2]}, cv[3] = {ka->cv[0], ka->cv[1], ka->cv[2]};
            const uint32_t px0 = nb_tx * kTileW, ly0 = nb_ty * kTileH;
            const uint32_t px1 = min(px0 + (kTileW - 1u), ka->W - 1u), ly1 = min(ly0 + (kTileH - 1u), ka->row_count - 1u);
            const rtwb::Beam beam =
                rtwb::tile_beam(org, llc, hor, ver, cu, cv, ka->lens_radius, ka->W, ka->H, px0, px1,
                                ka->row_begin + ly0 * ka->row_stride, ka->row_begin + ly1 * ka->row_stride);
            // TraceArgs::empty_on: the lanes after the slots answer for the wide spheres, lane n_slots + w for
            // the w-th of [0, g_static_wide) and [g_static, g_moving_wide), with their records of the same tables.
            bool may = false;
            const uint32_t n_slots = kClusterSlots * ka->sc.n_clusters;  // (primary_on: one 64-slot block)
            const uint32_t n_wide = ka->empty_on ? ka->sc.g_static_wide + (ka->sc.g_moving_wide - ka->sc.g_static) : 0u;
            if (lid < n_slots + n_wide) {
              uint32_t slot = lid;  // (laundered: the table's address is made here, not held across the loop)
              asm volatile("" : "+v"(slot));
              const uint32_t w = lid - n_slots;
              const uint32_t k = lid < n_slots ? T.cpos[slot]
                                               : (w < ka->sc.g_static_wide ? w : ka->sc.g_static + (w - ka->sc.g_static_wide));
              const uint32_t meta = T.meta[k];
              const bool mv = (meta & kMoving) != 0;
              const uint32_t g = mv ? (meta >> 2) & 63u : 0u;
              const double g0 = mv ? (double)T.tg[4 * g] : 0.0, g1 = mv ? (double)T.tg[4 * g + 1] : 1.0;
              const double c0[3] = {(double)T.sph[8 * k], (double)T.sph[8 * k + 1], (double)T.sph[8 * k + 2]};
              const double dc[3] = {(double)T.sph[8 * k + 3], (double)T.sph[8 * k + 4], (double)T.sph[8 * k + 5]};
              may = rtwb::beam_may_hit(beam, c0, dc, (double)T.rad[k], mv, g0, g1, ka->time0, ka->time1);
            }
            // bit j = slot j; the survivor loop wants slot 32h + r at bit 31 - r of word h
            const uint64_t bal = wballot(may && lid < n_slots);
            nb_bm0 = __builtin_bitreverse32((uint32_t)bal);
            nb_bm1 = __builtin_bitreverse32((uint32_t)(bal >> 32));
            // The tile's verdict: no camera ray of it can hit a sphere, real slot or wide (TraceArgs::empty_on).
            const RTW_CONST uint32_t* cval = cptr(ka->sc.cvalid);  // (dummy slots answer for table position 0)
            nb_empty = (ka->empty_on && ((nb_bm0 & cval[0]) | (nb_bm1 & cval[1])) == 0u &&
                        wballot(may && lid >= n_slots) == 0ull)
                           ? 1u
                           : 0u;
            cwd[2] = rtwc::pass_word(nb_ty * ka->tiles_x + nb_tx, nb_empty);
            cwd[3] = nb_bm0, cwd[4] = nb_bm1;
            if constexpr (STATS) {
              if (lid == 0 && base2 < RTW_KA(total_units)) st.beam_passes++;
            }
          }
          const RTW_CONST uint32_t* cval = cptr(ka->sc.cvalid);
          if (base2 < RTW_KA(total_units)) cwd[5] = rtwc::run_after(cwd[5], nb_empty);
          // (per fetched batch, its pass made or reused)
          if constexpr (STATS) {
            if (lid == 0 && base2 < RTW_KA(total_units)) st.mask_pop += __popc(nb_bm0 & cval[0]) + __popc(nb_bm1 & cval[1]);
          }
          // A batch no camera ray of which can hit a sphere (the host set empty_on
          // only with max_depth >= 1: at depth 0 a sample ends before its miss adds anything): every
          // sample of its units is bounce's miss with L.T = (1, 1, 1), so lane j finishes unit base2 + j here —
          // 0.0, + bg once per sample as that path adds it, stored as publish_unit stores — and the wave
          // fetches the next batch.  No lane's unit, ray or path changes; a lane waiting for a unit still is.
          if (nb_empty == 0u || base2 >= RTW_KA(total_units)) break;
          {
            const uint32_t l = dealt_unit(base2 + lid, *ka) & 63u;
            const uint32_t px = nb_tx * kTileW + (l & 7u), ly = nb_ty * kTileH + (l >> 3);
            if (px < ka->W && ly < ka->row_count) {  // else: a padding unit
              const uint32_t s0 = nb_c * ka->chunk, ns = min(s0 + ka->chunk, ka->spp) - s0;
              const double bg0 = (double)ka->bg[0], bg1 = (double)ka->bg[1], bg2 = (double)ka->bg[2];
              double z = 0.0;  // (laundered, as the take's)
              asm volatile("" : "+v"(z));
              double e0 = z, e1 = z, e2 = z;
#pragma unroll 1
              for (uint32_t i = 0; i < ns; ++i) e0 += bg0, e1 += bg1, e2 += bg2;
              double* dst = ka->partial + ((size_t)nb_c * (ka->row_count * ka->W) + (size_t)ly * ka->W + px) * 3;
              dst[0] = e0;
              dst[1] = e1;
              dst[2] = e2;
              if constexpr (STATS) st.samples += ns, st.segments += ns, st.empty_units++, st.empty_samples += ns;
            }
          }
        }
      }
      if (need) {
        const uint32_t unit = rank < rem ? qnext + rank : base2 + (rank - rem);
        if (unit >= RTW_KA(total_units)) {
          done = true;
        } else {
          const uint32_t du = dealt_unit(unit, *opaque(kargs<R>()));
          const uint32_t l = du & 63u;
          bool active = true;  // (MASKED)
          const uint32_t units_per_tile = kTileW * kTileH * RTW_KA(n_chunks);
          uint32_t tile = rtwm::udiv(du, RTW_KA(upt_m), RTW_KA(upt_sh));  // du / units_per_tile
          const uint32_t r = du - tile * units_per_tile;
          const uint32_t c = r >> 6;
          if constexpr (MASKED) {  // (unit < total_units: tile < the list's length)
            // Both pointers are read from the kernel argument here, in f32 too: held in SGPRs for the
            // whole kernel they cost the f32 kernel spills.  The frame has < 2^24 tiles (validate: <= 2^24
            // pixels), so the masked indices let the loads take a 32-bit offset.
            const auto* ka = opaque(kargs<R>());
            tile = ka->tile_list[tile & 0xFFFFFFu] & 0xFFFFFFu;
            // (the 32-bit half of the mask that holds bit l: one register less than the u64)
            const uint32_t half = reinterpret_cast<const uint32_t*>(ka->tile_mask)[2u * tile + (l >> 5)];
            active = ((half >> (l & 31u)) & 1u) != 0;
          }
          const uint32_t ty = rtwm::udiv(tile, RTW_KA(tx_m), RTW_KA(tx_sh));  // tile / tiles_x
          const uint32_t tx = tile - ty * RTW_KA(tiles_x);
          const uint32_t px = tx * kTileW + (l & 7u);
          const uint32_t ly = ty * kTileH + (l >> 3);
          if (px < RTW_KA(W) && ly < RTW_KA(row_count) && active) {  // else: padding or inactive unit, take another
            have_unit = true;
            L.s = c * RTW_KA(chunk);
            double z = 0.0;  // (laundered: a hoisted constant would hold registers)
            asm volatile("" : "+v"(z));
            h_u32[lid] = px;
            h_u32[64 + lid] = ly;
            h_u32[128 + lid] = c;
            h_u32[192 + lid] = min(L.s + RTW_KA(chunk), RTW_KA(spp));
            h_sum[lid] = h_sum[64 + lid] = h_sum[128 + lid] = z;
            if constexpr (PF) {  // the mask of the lane's own batch, current or new
              h_me[kPm] = rank < rem ? h_me[kBm] : nb_bm0;
              h_me[kPm + 64] = rank < rem ? h_me[kBm + 64] : nb_bm1;
            }
          }
        }
      }
      if (n > rem) {
        qnext = base2 + (n - rem);
        qend = base2 + kBatch;
        if constexpr (PF) {  // after the takes above read the old one
          h_me[kBm] = nb_bm0, h_me[kBm + 64] = nb_bm1;
        }
      } else {
        qnext += n;
      }
    }
  };

  // A finished sample joins its chunk sum (main.zig:393); a finished unit is
  // published.  (A miss added its colour; depth limit and absorption add 0.)
  auto publish_unit = [&]() __attribute__((always_inline)) {
    const uint32_t npix = RTW_KA(row_count) * RTW_KA(W);
    double* dst = RTW_KA(partial) +
                  ((size_t)h_u32[128 + lid] * npix + (size_t)h_u32[64 + lid] * RTW_KA(W) + h_u32[lid]) * 3;
    dst[0] = h_sum[lid];
    dst[1] = h_sum[64 + lid];
    dst[2] = h_sum[128 + lid];
    have_unit = false;
  };
  auto finish_sample = [&]() __attribute__((always_inline)) {
    L.s++;
    have_ray = false;
    if (STATS) st.samples++;
    if (L.s == h_u32[192 + lid]) publish_unit();
  };
  // One closest-hit step for a lane with a live ray (main.zig:103-112).
  // Returns 1 when the sample ended (depth limit or miss), 2 when the hit is
  // to be shaded.  (A result code, not two bool& outputs: the optimiser merged
  // their stores through a selected pointer, which put both flags in scratch
  // memory — a store + load per iteration on the critical path.)
  // prim (the primary-first loop): the lane's camera ray, from the mask of its tile
  // (closest_hit's PRIMARY form) instead of the wave's pretest.
  // (always_inline: with the loop body compiled twice its call sites are too many for the inliner)
  auto bounce = [&](uint32_t& kind, int& hit, R& tmax, auto prim) __attribute__((always_inline)) -> int {
    constexpr bool PRIM = decltype(prim)::value;
    if (L.depth == RTW_KA(max_depth)) {  // rayColor depth == 0 (main.zig:105-108)
      return 1;
    }
    if (STATS) st.segments++;
    if constexpr (STATS) {
      if (lid == (uint32_t)__builtin_ctzll(__ballot(true))) (PRIM ? st.prim_rounds : st.wave_iters)++;
    }
    uint32_t pm0 = 0u, pm1 = 0u;
    if constexpr (PRIM) pm0 = h_me[kPm], pm1 = h_me[kPm + 64];
    // (scene fields re-read from the kernel argument: SGPR budget)
    closest_hit<R, F32, MODE, PRIM, false, Cfg::kLeavePre>(opaque(kargs<R>())->sc, T, L, RTW_KA(tmin), RTW_KA(pre_k), lid,
                                                           st, hit, tmax, pm0, pm1);
    if (hit < 0) {  // miss: background (main.zig:109-112)
      const V3<R> col = mulv(L.T, ld3(opaque(kargs<R>())->bg));
      h_sum[lid] += (double)col.x;
      h_sum[64 + lid] += (double)col.y;
      h_sum[128 + lid] += (double)col.z;
      return 1;
    }
    kind = T.kind[(T.meta[hit] >> 8) & 0xFFFu];
    return 2;
  };

  bool primary_ran = false;
  if constexpr (PF) {
    if (A.primary_on) {
      // Primary-first loop (Cfg::kPrimaryFirst; TraceArgs::primary_on): [take
      // units] -> [new samples, per lane: u, v, the lens-disk point from the
      // lane's own loop, the camera ray and ITS closest hit — the wide spheres,
      // then the exact tests of the spheres in the mask of the lane's tile; a
      // miss ends the sample here] -> ONE coop pass: unit-ball points and
      // dielectric draws of the hits of this iteration's camera rays and of the
      // previous step's secondary rays -> [scatter] -> [closest hit of the
      // scattered rays through the wave's pretest].  A sample whose camera ray
      // hits takes one wave-iteration less than in the rotated loop; each
      // sample's draws are in the reference's order, and the exact tests, the
      // tie rule and the NaN fallback are closest_hit's.
      primary_ran = true;
      LaneFlag<8u> shading{lane_flags};
      LaneFlag<16u> helping{lane_flags};  // tail: the lane traces sample L.s of lane h_u32[128 + lid]'s unit
      uint32_t kind = 0;
      int hit = -1;
      R tmax = kInf;
      // The wave's tail block (TraceArgs::tail_on; after the wave's primary masks), words per lane:
      //   [lid]                the unit's first sample no lane has been given (`next`)
      //   [64 + lid]           nonzero while the lane traces or holds a sample of another lane's unit
      //   [128 + i]            the dealing list
      //   [192 + 64 j + lid]   the unit's window: 0x80 | helper lane of sample s, j = s % kTailWindow,
      //                        | 0x40 once that helper's h_sum triple holds the sample's radiance
      // The tail copy reaches it, and the other lanes' home entries, through wave_u32(): the wave's h_u32 made
      // from the lane's own h_me, so that no value of the tail lives in the bulk copy's registers.  (The lane
      // index is laundered, not the pointer: a laundered pointer is a generic one, 64 bits and flat accesses.)
      auto wave_u32 = [&]() -> uint32_t* {
        uint32_t l = lid;
        asm volatile("" : "+v"(l));
        return h_me - l;
      };
      constexpr uint32_t kTl = (uint32_t)((Cfg::kHomeStride - 3 * 64 * 8) / 4);  // the tail block, from h_u32
      auto tail_block = [&]() -> uint32_t* { return wave_u32() + kTl; };
      // The loop body, compiled twice (as rtw_world.hip's): without the tail for the bulk of the launch, and
      // with it once the queue ran dry for some lane of the wave.  Returns true when the wave has finished.
      // Tail (dealing on): the lanes left without a unit trace the NEXT samples of the wave's other units,
      // up to kTailWindow - 1 ahead of the owner's, each into its own (free) h_sum triple; the owner, after
      // the sample it traces itself, adds the finished ones in ascending sample order with finish_sample's
      // path's own additions (a sample that added nothing: + 0.0), starts nothing while the next sample in
      // order is in flight, and alone publishes the chunk sum.  The RNG state is a function of (pixel,
      // sample), so the sums keep their bits.
      // (always_inline: called twice, the body would stay a function, its captures in scratch memory)
      auto body = [&](auto tail_tag) __attribute__((always_inline)) -> bool {
        constexpr bool TAIL = decltype(tail_tag)::value;
        RTW_STAMP(5)
        // (the tail's per-lane `start` is a flag bit and `deal` is re-read where used: as variables they were
        // SGPRs held across the closest hits, spilled to VGPR lanes)
        LaneFlag<32u> start{lane_flags};
        auto deal = [&]() -> bool { return RTW_KA(tail_on) != 0u; };
        if constexpr (!TAIL) {
          take_units();
        } else {
          // (a wave takes its units in ascending order, and one lay past the queue's end: the next do too)
          if (!have_unit) done = true;
        }
        if (!__any(have_unit)) {
          if (__all(done)) return true;
          return false;
        }
        if constexpr (TAIL) {
          start = have_unit && !have_ray;
          if (deal()) {
            uint32_t* const tl = tail_block();
            // an owner takes its own next sample from `next` too, before any is handed out
            if (start) {
              if (tl[lid] == L.s)
                tl[lid] = L.s + 1u;
              else
                start = false;
            }
            for (;;) {
              wave_lds_sync();
              const bool free_lane = !have_unit && !helping && tl[64 + lid] == 0u;
              const uint64_t needm = wballot(free_lane);
              if (!needm) break;
              uint32_t nx = 0;
              bool offer = false;
              if (have_unit) {  // (L.s: the owner's sample in flight, or the first one not yet in its sum)
                nx = tl[lid];
                offer = nx < h_me[192] && nx < L.s + kTailWindow;
              }
              const uint64_t offm = wballot(offer);
              if (!offm) break;
              const uint32_t ro = mbcnt64(offm);
              if (offer) {
                tl[128 + ro] = lid | (nx << 6);
                if (ro < popc64(needm)) tl[lid] = nx + 1u;
              }
              wave_lds_sync();
              const uint32_t rw = mbcnt64(needm);
              if (free_lane && rw < popc64(offm)) {
                const uint32_t e = tl[128 + rw], o = e & 63u;
                helping = true;
                L.s = e >> 6;
                double z = 0.0;
                asm volatile("" : "+v"(z));
                const uint32_t* const ho = tl - kTl + o;  // the owner's home entries
                h_me[0] = ho[0];
                h_me[64] = ho[64];
                h_me[128] = o;
                h_me[kPm] = ho[kPm];
                h_me[kPm + 64] = ho[kPm + 64];
                h_sum[lid] = h_sum[64 + lid] = h_sum[128 + lid] = z;
                tl[64 + lid] = 1u;
                tl[192 + 64 * (L.s % kTailWindow) + o] = 0x80u | lid;
              }
            }
            if (helping && !have_ray) start = true;
          }
          if constexpr (STATS) {
            if (lid == (uint32_t)__builtin_ctzll(__ballot(true))) st.tail_iters++;
            if (!have_ray && !start) st.tail_idle++;
          }
        }
        // A finished sample: finish_sample, but in the dealing tail a helper leaves its sample's radiance in
        // its h_sum triple for the owner, and an owner's unit ends in the fold below.
        auto finish = [&]() {
          if constexpr (!TAIL) {
            finish_sample();
          } else if (!deal()) {
            finish_sample();
          } else {
            have_ray = false;
            if (STATS) st.samples++;
            if (helping) {
              helping = false;
              if (STATS) st.tail_helped++;
              tail_block()[192 + 64 * (L.s % kTailWindow) + h_me[128]] = 0xC0u | lid;
            } else {
              L.s++;
            }
          }
        };
        RTW_STAMP(0)
        // (at the loop's top a lane has a ray exactly when it is shading)
        // (the lens-disk point from the lane's own loop: 0.6 % faster than a disk-only cooperative pass
        // before the camera rays, profiles/r11/README.md)
        if (TAIL ? (bool)start : (have_unit && !have_ray)) {
          R u = (R)0, v = (R)0, dk[2] = {(R)0, (R)0};
          L.px = h_u32[lid];
          L.ly = h_u32[64 + lid];
          start_sample_uv<R>(kargs<R>(), L, u, v);
          for (;;) {  // randomPointInUnitDisk (rand.zig:30-36)
            dk[0] = rrange_m11<R>(L.rs);
            dk[1] = rrange_m11<R>(L.rs);
            if (in_unit_ball<R, 2>(dk)) break;
          }
          start_sample_ray<R>(kargs<R>(), L, u, v, dk[0], dk[1]);
          have_ray = true;
          if (bounce(kind, hit, tmax, std::true_type{}) == 1) {  // miss or depth limit
            finish();
            if (STATS) st.prim_idle++;
          } else {
            shading = true;
          }
        }
        RTW_STAMP(9)
        const uint32_t dim = shading ? (kind <= 2u ? 3u : 1u) : 0u;  // (as in the rotated loop below)
        R pt[3] = {(R)0, (R)0, (R)0}, raw = (R)0;
        if (__any(dim != 0u)) coop_reject_mixed<R>(dim, L.rs, pt, raw, slots, lid);
        RTW_STAMP(7)
        if (shading) {
          if (scatter_hit<R, F32, true>(T, L, hit, tmax, kind, pt, raw)) finish();  // absorbed
        }
        RTW_STAMP(8)
        shading = false;
        hit = -1;
        tmax = kInf;
        bool ended = false;
        if (have_ray) {
          const int b = bounce(kind, hit, tmax, std::false_type{});
          ended = b == 1;
          shading = b == 2;
        }
        RTW_STAMP(3)
        if (ended) finish();
        if constexpr (TAIL) {
          if (deal()) {
            // An owner between samples adds the finished samples that follow, in sample order, and frees
            // their lanes; its unit ends here.
            wave_lds_sync();
            if (have_unit && !have_ray) {
              uint32_t* const tl = tail_block();
              const uint32_t nx = tl[lid];
              while (L.s != nx) {  // sample L.s went to another lane
                const uint32_t w = tl[192 + 64 * (L.s % kTailWindow) + lid];
                if (!(w & 0x40u)) break;  // still in flight
                const uint32_t hl = w & 63u;
                const double* const hs = reinterpret_cast<const double*>(tl - kTl - 3 * 64 * 2) + hl;  // lane hl's triple
                h_sum[lid] += hs[0];
                h_sum[64 + lid] += hs[64];
                h_sum[128 + lid] += hs[128];
                tl[64 + hl] = 0u;
                L.s++;
              }
              if (L.s == h_me[192]) publish_unit();
            }
          }
        }
        return false;
      };
      // The bulk copy runs until the wave has finished or, in a launch with the tail, until one of its lanes
      // is done; the tail copy then runs to the wave's end (at once, if the bulk copy finished).  One way out
      // of the bulk loop: with two, the loop held more SGPRs and re-read the kernel-argument pointer from a
      // spill lane a dozen times per iteration.
      // (the counting pass runs the tail copy with dealing off too: its tail words)
      // (`done` first: tail_on is re-read from the kernel argument, a load and its wait)
      for (;;) {
        if (body(std::false_type{})) break;
        if (__any(done) && (STATS || RTW_KA(tail_on) != 0u)) break;
      }
      if (STATS || RTW_KA(tail_on) != 0u) {
        if (RTW_KA(tail_on) != 0u) {
          uint32_t* const tl = tail_block();
          tl[lid] = have_ray ? L.s + 1u : L.s;
          tl[64 + lid] = 0u;
        }
        while (!body(std::true_type{})) {
        }
      }
    }
  }
  if (!primary_ran) {
    // Rotated loop: [take units] -> [u, v of new samples] -> ONE coop pass:
    // lens-disk points (new samples) + unit-ball points (the Lambertian /
    // Metal hits of the previous step) -> [scatter; camera rays] -> [closest
    // hit].  A lane whose path missed starts its next sample in the next
    // iteration before that iteration's closest hit, as in the textbook order;
    // each sample's draws are in the reference's order.  The sample's time draw
    // and the dielectric's draw are made inside the same cooperative pass
    // (coop_reject_mixed `raw`).
    LaneFlag<8u> shading{lane_flags};
    uint32_t kind = 0;
    int hit = -1;
    R tmax = kInf;
    for (;;) {
      RTW_STAMP(5)
      take_units();
      if (!__any(have_unit)) {
        if (__all(done)) break;
        continue;
      }
      RTW_STAMP(0)
      const bool ns = have_unit && !have_ray;
      R u = (R)0, v = (R)0;
      if (ns) {
        L.px = h_u32[lid];
        L.ly = h_u32[64 + lid];
        start_sample_uv<R>(kargs<R>(), L, u, v);
      }
      RTW_STAMP(1)
      // dim: 3 unit ball (Lambertian, Metal), 1 the dielectric's draw, 2 lens disk (+ time)
      // LDISK: the primary-first kernel running this loop (primary_on clear) keeps its new samples' disk
      // points in each lane's own loop, as that kernel was measured (in this loop alone 4.8 % slower than
      // the cooperative disk: profiles/r06/mk_var_ab.txt).
      constexpr bool LDISK = PF;
      const uint32_t dim = shading ? (kind <= 2u ? 3u : 1u) : (ns && !LDISK ? 2u : 0u);
      R pt[3] = {(R)0, (R)0, (R)0}, raw = (R)0;
      if (__any(dim != 0u)) coop_reject_mixed<R>(dim, L.rs, pt, raw, slots, lid);
      RTW_STAMP(7)
      if (shading) {
        if (scatter_hit<R, F32, true>(T, L, hit, tmax, kind, pt, raw)) finish_sample();  // absorbed
      }
      if (ns) {
        if constexpr (LDISK) {
          R dk[2];
          for (;;) {  // randomPointInUnitDisk (rand.zig:30-36)
            dk[0] = rrange_m11<R>(L.rs);
            dk[1] = rrange_m11<R>(L.rs);
            if (in_unit_ball<R, 2>(dk)) break;
          }
          start_sample_ray<R>(kargs<R>(), L, u, v, dk[0], dk[1]);
        } else {
          start_sample_ray<R, true>(kargs<R>(), L, u, v, pt[0], pt[1], raw);
        }
        have_ray = true;
      }
      RTW_STAMP(8)
      shading = false;
      hit = -1;
      tmax = kInf;
      bool ended = false;
      if (have_ray) {
        const int b = bounce(kind, hit, tmax, std::false_type{});
        ended = b == 1;
        shading = b == 2;
      }
      RTW_STAMP(3)
      if (ended) finish_sample();
    }
  }
  if (STATS) {
    atomicAdd(A.stats + 0, st.samples);
    atomicAdd(A.stats + 1, st.segments);
    atomicAdd(A.stats + 2, st.skipped);
    atomicAdd(A.stats + 3, st.candwave);
    atomicAdd(A.stats + 4, st.candlane);
    atomicAdd(A.stats + 5, st.disc);
    atomicAdd(A.stats + 6, st.wave_iters);
    atomicAdd(A.stats + 7, st.cull_lanes);
    atomicAdd(A.stats + 8, st.cull_iters);
    atomicAdd(A.stats + 11, st.cl_tests);
    atomicAdd(A.stats + 12, st.cl_skips);
    if constexpr (PF) {
      atomicAdd(A.stats + 14, st.prim_rounds);
      atomicAdd(A.stats + 15, st.prim_idle);
      atomicAdd(A.stats + 16, st.mask_pop);
      atomicAdd(A.stats + 17, st.tail_helped);
      atomicAdd(A.stats + 18, st.tail_iters);
      atomicAdd(A.stats + 19, st.tail_idle);
      atomicAdd(A.stats + 20, st.empty_units);
      atomicAdd(A.stats + 21, st.empty_samples);
      atomicAdd(A.stats + 22, st.claims);
      atomicAdd(A.stats + 23, st.beam_passes);
    }
  }
  if constexpr (MODE == 2) {
    RTW_STAMP(4)
    if (lid == 0)
      for (int i = 0; i < 10; ++i) atomicAdd(A.stats + 16 + i, (unsigned long long)st.ph[i]);
  }
}

// Chunk sums added in order, then main.zig:395-400 quantisation.
__global__ void __launch_bounds__(256) finalize_kernel(FinalizeArgs F) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < F.npix; i += gridDim.x * blockDim.x) {
    double t[3] = {0.0, 0.0, 0.0};
    for (uint32_t c = 0; c < F.n_chunks; ++c) {
      const double* p = F.partial + ((size_t)c * F.npix + i) * 3;
      t[0] += p[0];
      t[1] += p[1];
      t[2] += p[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double g = sqrt(t[k] * F.scale);
      const double cl = fmax(0.0, fmin(g, 0.999));
      F.rgb[(size_t)i * 3 + k] = (uint8_t)(256.0 * cl);
      if (F.mean) F.mean[(size_t)i * 3 + k] = (float)(t[k] * F.scale);
    }
  }
}

template <typename R, bool F32>
static hipError_t launch_trace(const TraceArgs<R>& a, uint32_t grid, size_t lds, hipStream_t s, int mode,
                               bool masked) {
  if (masked) {  // a masked accumulator pass (product mode only)
    if (mode != 0 || !a.tile_list || !a.tile_mask) return hipErrorInvalidValue;
    hipLaunchKernelGGL((trace_kernel<R, F32, 0, true>), dim3(grid), dim3(kTraceBlock), lds, s, a);
  } else if (mode == 1) {
    hipLaunchKernelGGL((trace_kernel<R, F32, 1, false>), dim3(grid), dim3(kTraceBlock), lds, s, a);
#ifdef RTW_MEASURE  // per-phase s_memtime stamps (diagnostic)
  } else if (mode == 2) {
    hipLaunchKernelGGL((trace_kernel<R, F32, 2, false>), dim3(grid), dim3(kTraceBlock), lds, s, a);
#endif
  } else {
    hipLaunchKernelGGL((trace_kernel<R, F32, 0, false>), dim3(grid), dim3(kTraceBlock), lds, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_trace_f64(const TraceArgs<double>& a, uint32_t grid, size_t lds, hipStream_t s, int mode,
                            bool masked) {
  return launch_trace<double, false>(a, grid, lds, s, mode, masked);
}
hipError_t launch_trace_f32(const TraceArgs<float>& a, uint32_t grid, size_t lds, hipStream_t s, int mode,
                            bool masked) {
  return launch_trace<float, true>(a, grid, lds, s, mode, masked);
}
hipError_t launch_finalize(const FinalizeArgs& a, hipStream_t s) {
  const uint32_t grid = min((a.npix + 255u) / 256u, 4096u);
  hipLaunchKernelGGL(finalize_kernel, dim3(grid ? grid : 1), dim3(256), 0, s, a);
  return hipGetLastError();
}

// f(std::bool_constant<F32>, std::bool_constant<MASKED>) for a launch's (precision, masked)
template <typename F>
static auto with_cfg(int precision, bool masked, F f) {
  if (precision == 1) return masked ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
  return masked ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}
int trace_blocks_per_cu(int precision, size_t lds, bool masked) {
  const int nb = with_cfg(precision, masked, [&](auto f32, auto m) {
    using R = std::conditional_t<f32.value, float, double>;
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, trace_kernel<R, f32.value, 0, m.value>, kTraceBlock, lds) !=
        hipSuccess)
      n = 0;
    return n;
  });
  return nb > 0 ? nb : 1;
}
bool trace_primary_first(int precision, bool masked) {
  return with_cfg(precision, masked, [](auto f32, auto m) { return TraceCfg<f32.value, m.value>::kPrimaryFirst; });
}
size_t trace_home_lds_bytes(int precision, bool masked) {
  return 8 + (kTraceBlock / 64) *
                 with_cfg(precision, masked, [](auto f32, auto m) { return TraceCfg<f32.value, m.value>::kHomeStride; });
}
size_t trace_tail_lds_bytes(int precision, bool masked) {
  return (kTraceBlock / 64) *
         with_cfg(precision, masked, [](auto f32, auto m) { return TraceCfg<f32.value, m.value>::kTailBytes; });
}

}  // namespace rtwk
