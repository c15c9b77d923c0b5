// rtw_world.hip — the general-world kernel: the reference's render loop and
// rayColor (main.zig:378-402, :103-122, emission included) over the full
// Hittable vocabulary (hittable.zig:22-608: spheres, moving spheres, xy/xz/yz
// rects, boxes, Translate, RotateY), all materials (material.zig:16-121,
// DiffuseLight included) and textures (texture.zig:10-144: solid, checker,
// Perlin noise, image), for every scene of main.zig and BASELINE.json
// configs[4] (globe + 10k spheres).  f64, the reference's arithmetic.
//
// Closest hit: wave-cooperative BVH2 traversal (both child boxes in the
// parent node; one stack per wave in LDS; scalar-loaded nodes and
// primitives), or a wave-uniform linear loop for small worlds.  The reference's HittableList.hit picks the object of
// minimal effective root, ties to the later object — an order-independent
// rule — so visiting primitives in BVH order returns the
// same winner as long as no box that could hold a winner is pruned: every
// box test is widened by `margin` (rtw_world_capi.hip bvh_margin: > the
// largest deviation of a computed root from the exact intersection) and is
// inclusive at tmax.  A NaN root (the reference's acceptance is then order
// dependent) sends the lane through the literal sequential loop.
//
// Per lane: the megakernel's work units (pixel, chunk of samples) with
// lane-level regeneration; per sample: the Tier-B counter RNG, rayColor
// evaluated forward (rad += T * emitted at a light, rad += T * background on a
// miss).  oracle/rtw_world.h Tier B is the written contract.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rtw_device.hpp"
#include "rtw_guides.hpp"
#include "rtw_libm.hpp"
#include "rtw_world_tex.hpp"
#include "rtw_world_walk.hpp"

// (Measured choices that are now the only code: the BVH stack's top entry in a
// register, profiles/r02/world_topcache_ab.txt; the node visit's decisions as
// scalar refs made before its leaf tests, profiles/r04/world_decide_refs_ab.txt;
// the lane's state flags as bits of one word, profiles/r04/world_lane_flags_ab.txt;
// the left child's record line touched with every node visit,
// profiles/r04/world_touch_next_ab.txt.)

namespace rtwk {


// (Texture.value over the tables, tex_value: rtw_world_tex.hpp, shared with rtw_surface.hip)

// The world's feature buffers (rtw_hip.h rtw_world_guides_device, DESIGN.md
// §14): one lane per pixel, the pixel's feature ray through the reference's
// literal sequential loop (seq_hit: no BVH, no LDS — the kernel runs once per
// frame, and the loop is the one traversal with nothing to get wrong), then the
// winner's hit record and texture value as world_kernel's shade computes them.
// The general feature set: every primitive, texture and transform (FEAT: kFeatAll, with kFeatTri for a
// world that holds triangles).
template <int FEAT>
__global__ void __launch_bounds__(kGuideTileW* kGuideTileH) world_guides_kernel(WorldGuideArgs A) {
  uint32_t x, q;
  if (!guide_pixel(A.r, x, q)) return;
  const WorldView& W = A.w;
  V o0, d0;
  guide_ray(A.r, x, q, o0, d0);
  const D time = A.r.time;
  WHit h;
  h.nan = 0u;
  seq_hit<FEAT>(W, W.order, o0, d0, time, (D)0.001, h);
  if (h.pos < 0) {
    guide_store(A.r, x, q, mk(0.0, 0.0, 0.0), 0.0, ld3(A.r.bg), 0u);
    return;
  }
  const uint32_t* mt = meta_of(W.prim + kWorldRec * h.pos);
  const D* mp = W.mat + 8 * mt[1];
  const uint32_t* mh = reinterpret_cast<const uint32_t*>(mp);
  const uint32_t mkind = mh[0], mtex = mh[1];
  const bool image_tex =
      (mkind == 0u || mkind == 3u) && *reinterpret_cast<const uint32_t*>(W.tex + kWorldRec * mtex) == 3u;
  // (getSphereUv only where an image texture reads it)
  const HitRec R = hit_record<FEAT>(W, h.pos, h.t, o0, d0, time, image_tex);
  const V& p = R.p;
  const V& nrm = R.nrm;
  const D tu = R.u, tv = R.v;
  V albedo;
  if (mkind == 1u)
    albedo = ld3(mp + 1);
  else if (mkind == 2u)
    albedo = mk(1.0, 1.0, 1.0);
  else
    albedo = tex_value<FEAT>(W, mtex, tu, tv, p);
  guide_store(A.r, x, q, nrm, h.t, albedo, (uint32_t)h.orig + 1u);
}

hipError_t launch_world_guides(const WorldGuideArgs& a, bool tri, hipStream_t s) {
  const dim3 grid((a.r.W + kGuideTileW - 1) / kGuideTileW, (a.r.row_count + kGuideTileH - 1) / kGuideTileH);
  if (tri)
    hipLaunchKernelGGL(world_guides_kernel<kFeatAll | kFeatTri>, grid, dim3(kGuideTileW * kGuideTileH), 0, s, a);
  else
    hipLaunchKernelGGL(world_guides_kernel<kFeatAll>, grid, dim3(kGuideTileW * kGuideTileH), 0, s, a);
  return hipGetLastError();
}

// OCC: minimum resident workgroups per CU asked of the register allocator
// (1 = unconstrained; chosen by A/B on MI355X, rtw_world_capi.hip).
template <int MODE, int OCC, int FEAT>
__global__ void __launch_bounds__(kWorldBlock, OCC) world_kernel(WorldArgs A) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  // this wave's BVH stack: one column per lane (per-lane traversal) or one
  // wave-uniform stack (the union walk)
  uint32_t* stack = reinterpret_cast<uint32_t*>(lds_raw) +
                    (threadIdx.x >> 6) * ((FEAT & kFeatLane) ? kLaneWaveWords : kBvhStack);
  // per-lane traversal: this wave's LaneTrav rows follow its stack columns,
  // and the lanes' attenuation rows (T) follow them
  LaneTravRows* trav_rows = reinterpret_cast<LaneTravRows*>(stack + kLaneStackLds * 64u);
  double(*t_rows)[64] = reinterpret_cast<double(*)[64]>(stack + (kLaneStackLds + kTravWords) * 64u);
  // the per-lane walk's node cache (packed refs): the top kNodeCache records, words 0-11
  constexpr bool NCACHE = (FEAT & kFeatLane) != 0 && (FEAT & kFeatPacked) != 0 && kNodeCache > 0;
  const nf4* node_cache = nullptr;  // (staged below; no LDS at all when NCACHE is off)
  // Tail dealing rows of this wave's lanes (lane = the owner of a unit): the
  // first sample handed to other lanes (samples [hi, s_end) are theirs), the
  // ring entries they filled, the unit's pixel; and the dealing list.
  // (Row addresses formed at each use from the wave-uniform index: held as
  // pointers they cost registers across the whole loop.)
  __shared__ uint32_t tail_rows[kWorldBlock / 64][5][64];
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#define TL_HI tail_rows[wv][0]
#define TL_READY tail_rows[wv][1]
#define TL_PXLY tail_rows[wv][2]
#define TL_LIST tail_rows[wv][3]
#define TL_OWN tail_rows[wv][4]  // a helper's owner lane
#define TL_C tail_rows[wv][4]    // an owner's chunk (one row: a lane helps only once it owns no unit)
  // The lane's f64 chunk sum (a helper's: the radiance of the sample it
  // traces) lives in LDS too: it changes only when a sample ends.
  __shared__ double home_sum[kWorldBlock / 64][3][64];
#define HS(k) home_sum[wv][k][lid]
  // (The unit's pixel and chunk live only in these rows, read where used —
  // sample start, chunk-sum publish — instead of VGPRs across the loop.)
  // The world's fields are re-read from the kernel argument where used
  // (scalar loads through a laundered kernarg pointer) instead of living in
  // SGPRs for the whole kernel: at the 100-SGPR limit they spill to VGPR
  // lanes (v_writelane / v_readlane in the traversal loop).  As the
  // megakernel's scene fields (rtw_trace.hip bounce); +1.4 % on the
  // globe and Cornell (profiles/r02/world_karg_ab.txt).
  const RTW_CONST WorldView& W =
      opaque((const RTW_CONST WorldArgs*)__builtin_amdgcn_kernarg_segment_ptr())->w;
  // The loop's other argument fields too (as the megakernel's TraceCfg::kLoopArgsFromKernarg):
  // read where used, through the same laundered pointer.
#define WKA(f) (opaque((const RTW_CONST WorldArgs*)__builtin_amdgcn_kernarg_segment_ptr())->f)
  const uint32_t* order = W.order;
  const uint32_t lid = lane_id();
  if constexpr (NCACHE) {  // stage the node cache (every thread reaches this before the persistent loop)
    __shared__ nf4 ncache_lds[(kNodeCache > 0 ? kNodeCache : 1u) * 3u];
    const uint32_t nn = min(W.n_nodes, kNodeCache);
    const nf4* gn = reinterpret_cast<const nf4*>(W.node);
    for (uint32_t i = threadIdx.x; i < 3u * nn; i += kWorldBlock) ncache_lds[i] = gn[(i / 3u) * 4u + i % 3u];
    __syncthreads();
    node_cache = ncache_lds;
  }
  Lane<D> L;
  L.px = L.ly = L.c = L.s = L.s_end = L.depth = 0;
  L.rs = 0;
  L.skip = -1;
  // The path attenuation T (rayColor's product of attenuations, main.zig:117)
  // of the per-lane kernel lives in LDS rows: it changes only when a segment
  // is shaded, and held in VGPRs across the BVH walk it was what the 4-wave
  // budget spilled (written back every iteration of the persistent loop).
  auto t_get = [&]() -> V {
    if constexpr ((FEAT & kFeatLane) != 0) return mk(t_rows[0][lid], t_rows[1][lid], t_rows[2][lid]);
    return L.T;
  };
  auto t_set = [&](const V& v) {
    if constexpr ((FEAT & kFeatLane) != 0) {
      t_rows[0][lid] = v.x, t_rows[1][lid] = v.y, t_rows[2][lid] = v.z;
    } else {
      L.T = v;
    }
  };
  // rayColor forward (main.zig:103-122): a sample's radiance is nonzero only at
  // the event that ends it (a miss adds T * background, a light T * emitted),
  // so that one term joins the chunk sum directly: sx + (0 + x) == sx + x
  // (x >= +0), the oracle's `rad` (rtw_world.c sample_b) without its registers.
  // The lane's state flags as bits of ONE word (a VGPR): as bools, each was a
  // 64-bit lane mask in SGPRs for the whole loop, and at the traversal's SGPR
  // peak the compiler spilled SGPRs to VGPR lanes (v_writelane / v_readlane,
  // VALU instructions) around it.
  uint32_t lane_flags = 0u;
  LaneFlag<1u> have_unit{lane_flags};
  LaneFlag<2u> have_ray{lane_flags};
  LaneFlag<4u> done{lane_flags};
  LaneFlag<8u> waiting{lane_flags};   // owner: its own samples done, waiting for the ones other lanes trace
  LaneFlag<16u> helping{lane_flags};  // helper: traces sample L.s of lane TL_OWN[lid]'s unit
  LaneFlag<32u> walking{lane_flags};  // per-lane traversal: a paused BVH walk (state in its LaneTrav row)
  uint32_t qnext = 0, qend = 0;
  unsigned long long n_samples = 0, n_segments = 0, n_visits = 0, n_tests = 0, n_iters = 0;
  unsigned long long n_wi = 0, n_wl = 0;  // per-lane traversal: interior / leaf wave iterations
  KStats st;  // MODE 2: phase stamps
  if constexpr (MODE == 2) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st.t_last)::"memory");
  // The loop body, compiled twice: without the tail dealing for the bulk of
  // the launch, and with it once the queue ran dry for some lane of the wave
  // (its variables then are not live in the bulk loop's register allocation).
  // Returns 1 when every lane is done.
  auto body = [&](auto tail_tag) -> int {
    constexpr bool TAIL = decltype(tail_tag)::value;
    if (MODE == 1) ++n_iters;  // wave iterations (lane utilisation = segments / (64 x iterations))
    // ---- take units (wave-uniform; rtw_trace.hip step 1) ----
    const bool need = !have_unit && !done;
    const uint64_t needmask = __ballot(need);
    if (needmask) {
      const uint32_t n = (uint32_t)__popcll(needmask);
      const uint32_t rank = mbcnt64(needmask);
      const uint32_t rem = qend - qnext;
      uint32_t base2 = 0;
      if (n > rem) {
        uint32_t b = 0;
        if (lid == 0) b = atomicAdd(WKA(t.counter), kBatch);
        base2 = __shfl(b, 0);
      }
      if (need) {
        const uint32_t raw = rank < rem ? qnext + rank : base2 + (rank - rem);
        if (raw >= WKA(t.total_units)) {
          done = true;
        } else {
          const uint32_t unit = dealt_unit(raw, WKA(t));
          const uint32_t units_per_tile = kTileW * kTileH * WKA(t.n_chunks);
          uint32_t tile = rtwm::udiv(unit, WKA(t.upt_m), WKA(t.upt_sh));  // unit / units_per_tile
          const uint32_t r = unit - tile * units_per_tile;
          // A masked accumulator pass (TraceArgs::tile_list; wave-uniform null check): the dealt tile
          // counts the active tiles, and the unit of an inactive pixel is skipped as a padding unit is.
          // Product mode only (accumulator passes run in no other): the counts and phase builds keep
          // their code.
          bool active = true;
          if constexpr (MODE == 0) {
            const uint32_t* tile_list = WKA(t.tile_list);
            if (tile_list != nullptr) {  // (raw < total_units: tile < the list's length)
              tile = tile_list[tile];
              const uint32_t l = r & 63u;
              const uint32_t half = reinterpret_cast<const uint32_t*>(WKA(t.tile_mask))[2u * tile + (l >> 5)];
              active = ((half >> (l & 31u)) & 1u) != 0;
            }
          }
          const uint32_t tiles_x = WKA(t.tiles_x);
          const uint32_t ty = rtwm::udiv(tile, WKA(t.tx_m), WKA(t.tx_sh)), tx = tile - ty * tiles_x;
          const uint32_t px = tx * kTileW + ((r & 63u) & 7u), ly = ty * kTileH + ((r & 63u) >> 3);
          if (px < WKA(t.W) && ly < WKA(t.row_count) && active) {
            have_unit = true;
            L.s = (r >> 6) * WKA(t.chunk);
            TL_C[lid] = r >> 6;
            L.s_end = min(L.s + WKA(t.chunk), WKA(t.spp));
            HS(0) = HS(1) = HS(2) = 0.0;
            TL_HI[lid] = L.s_end;
            TL_READY[lid] = 0u;
            TL_PXLY[lid] = px | (ly << 16);
          }
        }
      }
      if (n > rem) {
        qnext = base2 + (n - rem);
        qend = base2 + kBatch;
      } else {
        qnext += n;
      }
    }
    if (!__any(have_unit)) {
      if (__all(done)) return 1;
      return 0;
    }
    // ---- tail: once the queue ran dry for some lane of the wave, the lanes
    // left without a unit trace the LAST samples of the wave's other units
    // (one per offering unit per pass, up to kTailWin of a unit), each
    // sample's radiance going to its owner's ring; an owner stops at the
    // first sample it handed out and folds the ring in sample order
    // (main.zig:393), the other engines' addition sequence.  A world unit
    // runs ~84 wave iterations, so without this the launch ends with lanes
    // idle while the last units finish.
    constexpr bool tail = TAIL;
    if constexpr (tail) {
      for (;;) {
        const bool free_lane = done && !have_unit && !helping;
        const uint64_t needm = wballot(free_lane);
        if (!needm) break;
        uint32_t hi = 0;
        bool offer = false;
        if (have_unit && !waiting) {  // (L.s: the sample in flight or the next to start)
          hi = TL_HI[lid];
          offer = hi > max(L.s + 1u, L.s_end > kTailWin ? L.s_end - kTailWin : 0u);
        }
        const uint64_t offm = wballot(offer);
        if (!offm) break;
        const uint32_t ro = mbcnt64(offm);
        if (offer) {
          TL_LIST[ro] = lid | ((hi - 1u) << 6);
          if (ro < popc64(needm)) TL_HI[lid] = hi - 1u;
        }
        wave_lds_sync();
        const uint32_t rw = mbcnt64(needm);
        if (free_lane && rw < popc64(offm)) {
          const uint32_t e = TL_LIST[rw];
          helping = true;
          TL_OWN[lid] = e & 63u;
          L.s = e >> 6;
          HS(0) = HS(1) = HS(2) = 0.0;
        }
        wave_lds_sync();
      }
    }
    // ---- new sample ----
    if (((have_unit && !waiting) || helping) && !have_ray) {
      D u, v, dk[2];
      const uint32_t pl = TL_PXLY[helping ? TL_OWN[lid] : lid];  // the unit's pixel (this lane's or its owner's)
      L.px = pl & 0xFFFFu;
      L.ly = pl >> 16;
      start_sample_uv<D>(kargs<D>(), L, u, v);
      for (;;) {  // randomPointInUnitDisk, rand.zig:30-36
        dk[0] = rrange_m11<D>(L.rs);
        dk[1] = rrange_m11<D>(L.rs);
        if (in_unit_ball<D, 2>(dk)) break;
      }
      start_sample_ray<D>(kargs<D>(), L, u, v, dk[0], dk[1]);
      t_set(L.T);  // (= 1, 1, 1: start_sample_ray)
      have_ray = true;
    }
    // ---- one segment ----
    bool ended = false;
    // The hit record, texture and scatter of a lane whose closest hit is h
    // (written once, used by both traversals).
    auto shade = [&](WHit& h) {
      if (__builtin_expect(h.nan != 0u, 0)) seq_hit<FEAT>(W, order, L.o, L.d, L.time, WKA(t.tmin), h);
      if (h.pos < 0) {  // miss: background (main.zig:109-112)
        const V c = mulv(t_get(), ld3(opaque(kargs<D>())->bg));
        HS(0) += c.x;
        HS(1) += c.y;
        HS(2) += c.z;
        ended = true;
      } else {
        // Hit record of the winner (object space, then the wrappers back).
        const D* r = W.prim + kWorldRec * h.pos;
        const uint32_t* mt = meta_of(r);
        const uint32_t kind = mt[0] & 0xFFu;
        const int xf = (int)(mt[0] >> 8) - 1;
        V o = L.o, d = L.d;
        if ((FEAT & kFeatXform) && xf >= 0) to_object(W.xform + kWorldRec * xf, o, d);
        V p = add(o, mul(d, h.t)), nrm;
        bool front;
        D tu = 0.0, tv = 0.0;
        const D* mp = W.mat + 8 * mt[1];
        const uint32_t* mh = reinterpret_cast<const uint32_t*>(mp);
        const uint32_t mkind = mh[0], mtex = mh[1];
        const bool image_tex = (FEAT & kFeatImage) &&
            (mkind == 0u || mkind == 3u) && *reinterpret_cast<const uint32_t*>(W.tex + kWorldRec * mtex) == 3u;
        if ((FEAT & kFeatTri) && kind == 5u) {  // rtw_tri.hpp (as hit_record)
          const V n0 = mk(r[rtwtri::kNx], r[rtwtri::kNy], r[rtwtri::kNz]);
          if (image_tex) rtwtri::bary(r, o.x, o.y, o.z, d.x, d.y, d.z, tu, tv);  // (only an image texture reads u, v)
          front = dot(n0, d) < 0.0;
          nrm = front ? n0 : mul(n0, -1.0);
        } else if (!(FEAT & kFeatRect) || kind <= 1u) {
          V c = ld3(r);
          if (kind == 1u) c = add(c, mul(ld3(r + 3), (L.time - r[7]) / r[8]));
          const V outward = divs(sub(p, c), r[6]);
          front = dot(outward, d) < 0.0;
          nrm = front ? outward : mul(outward, -1.0);
          if (kind == 0u && image_tex) {  // getSphereUv (hittable.zig:145-150)
            const D pi = 3.14159265358979323846;
            tu = (rtwl::atan2(-outward.z, outward.x) + pi) / (2.0 * pi);
            tv = rtwl::acos(-outward.y) / pi;
          }
        } else {
          D oa, ob, da, db;
          V n0;
          if (kind == 2u) {
            oa = o.x, ob = o.y, da = d.x, db = d.y, n0 = mk(0.0, 0.0, 1.0);
          } else if (kind == 3u) {
            oa = o.x, ob = o.z, da = d.x, db = d.z, n0 = mk(0.0, 1.0, 0.0);
          } else {
            oa = o.y, ob = o.z, da = d.y, db = d.z, n0 = mk(1.0, 0.0, 0.0);
          }
          tu = (oa + h.t * da - r[0]) / r[5];
          tv = (ob + h.t * db - r[2]) / r[6];
          front = dot(n0, d) < 0.0;
          nrm = front ? n0 : mul(n0, -1.0);
        }
        if ((FEAT & kFeatXform) && xf >= 0) to_world(W.xform + kWorldRec * xf, p, nrm);
        if (mkind == 3u) {  // DiffuseLight: emitted, no scatter (material.zig:94-110)
          const V c = mulv(t_get(), tex_value<FEAT>(W, mtex, tu, tv, p));
          HS(0) += c.x;
          HS(1) += c.y;
          HS(2) += c.z;
          ended = true;
        } else {
          V ndir, att;
          bool absorbed = false;
          // Lambertian and Metal draw their unit-ball point in ONE per-lane
          // rejection loop (randomPointInUnitSphere, rand.zig:22-28; the wave
          // would otherwise run the two loops one after the other), and every
          // lane makes one normalisation: the ball point (Lambertian) or the
          // ray direction (Metal, Dielectric).  Same draws, same operations.
          D b3[3] = {0.0, 0.0, 0.0};
          if (mkind <= 1u) {
            for (;;) {
              b3[0] = rrange_m11<D>(L.rs);
              b3[1] = rrange_m11<D>(L.rs);
              b3[2] = rrange_m11<D>(L.rs);
              if (in_unit_ball<D, 3>(b3)) break;
            }
          }
          const V nv = normalized(mkind == 0u ? mk(b3[0], b3[1], b3[2]) : L.d);
          if (mkind == 0u) {  // Lambertian (material.zig:44-52)
            ndir = add(nrm, nv);
            if (fabs(ndir.x) < 1e-8 && fabs(ndir.y) < 1e-8 && fabs(ndir.z) < 1e-8) ndir = nrm;
            att = tex_value<FEAT>(W, mtex, tu, tv, p);
          } else {
            // reflect(ud, nrm) (material.zig:112-114) for Metal and Dielectric;
            // the Dielectric's dot(-ud, nrm) (:75) is exactly -dun
            const V& ud = nv;
            const D dun = dot(ud, nrm);
            const V refl = sub(ud, mul(nrm, 2 * dun));
            if (mkind == 1u) {  // Metal (material.zig:59-65)
              ndir = add(refl, mul(mk(b3[0], b3[1], b3[2]), mp[4]));
              att = ld3(mp + 1);
              absorbed = !(dot(refl, nrm) > 0.0);
            } else {  // Dielectric (material.zig:72-91)
              const D ir = mp[5];
              const D ratio = front ? 1.0 / ir : ir;
              const D cos_t = fmin(-dun, 1.0);
              const D sin_t = sqrt(1.0 - cos_t * cos_t);
              bool refr = false;
              if (ratio * sin_t <= 1.0) {
                const D r0 = (1.0 - ratio) / (1.0 + ratio);
                const D r1 = r0 * r0;
                const D x = 1.0 - cos_t, x2 = x * x;
                refr = r1 + (1.0 - r1) * (x * (x2 * x2)) < rnd<D>(L.rs);  // Zig pow(x, 5.0)
              }
              if (refr) {  // refract (:116-121); its cos_theta is cos_t
                const V perp = mul(add(ud, mul(nrm, cos_t)), ratio);
                ndir = add(perp, mul(nrm, -sqrt(fabs(1.0 - norm2(perp)))));
              } else {
                ndir = refl;
              }
              att = mk(1.0, 1.0, 1.0);
            }
          }
          if (absorbed) {
            ended = true;
          } else {
            t_set(mulv(t_get(), att));
            L.o = p;
            L.d = ndir;
            L.depth++;
          }
        }
      }
    };
    if constexpr ((FEAT & kFeatLane) != 0) {
      if (have_ray && !walking) {
        if (L.depth == WKA(t.max_depth)) {
          ended = true;  // rayColor(depth == 0) is black (main.zig:105-108)
        } else {
          walking = true;
          trav_begin(trav_rows, lid);
          if (MODE == 1) ++n_segments;
        }
      }
      WSTAMP(1)  // sample start (+ take units, loop control)
      // (walks yield in the tail copy of the loop too: the lanes that stopped
      // walking then take the wave's other units' samples.  A `wall(done)` test
      // here never held while a lane walked — a done lane without a unit only
      // walks as a helper, and helpers exist only while an owner, not done,
      // holds its unit: ADVICE r5 — and is gone.)
      const uint32_t yl = WKA(lane_yield);
      WHit h;
      if (trav_phase<MODE, FEAT>(W, WKA(margin), stack, trav_rows, node_cache, lid, walking, yl, L.o, L.d, L.time, WKA(t.tmin),
                                 h, n_visits, n_tests, n_wi, n_wl)) {
        walking = false;
        shade(h);
      }
    } else if (have_ray) {
      if (L.depth == WKA(t.max_depth)) {
        ended = true;  // rayColor(depth == 0) is black (main.zig:105-108)
      } else {
        if (MODE == 1) ++n_segments;
        WHit h;
        WSTAMP(1)  // sample start (+ take units, loop control)
        closest<MODE, FEAT>(W, WKA(margin), stack, L.o, L.d, L.time, WKA(t.tmin), h, n_visits, n_tests, st);
        shade(h);
      }
    }
    WSTAMP(4)  // hit record, texture, scatter (+ the NaN fallback)
    if (ended && helping) {  // a sample of another lane's unit: its radiance to that lane's ring
      const uint32_t j = L.s % kTailWin, o = TL_OWN[lid];
      double* rg = WKA(ring) + ((size_t)(blockIdx.x * kWorldBlock + wv * 64u + o) * kTailWin + j) * 3;
      rg[0] = HS(0);
      rg[1] = HS(1);
      rg[2] = HS(2);
      atomicOr(&TL_READY[o], 1u << j);
      helping = false;
      have_ray = false;
      if (MODE == 1) ++n_samples;
    } else if (ended) {  // (its radiance joined the chunk sum above, main.zig:393)
      L.s++;
      have_ray = false;
      if (MODE == 1) ++n_samples;
      if (L.s != L.s_end && tail && L.s == TL_HI[lid]) waiting = true;  // the rest went to other lanes
      if (L.s == L.s_end) {
        const uint32_t npix = WKA(t.row_count) * WKA(t.W);
        const uint32_t pl = TL_PXLY[lid];
        double* dst = WKA(t.partial) + ((size_t)TL_C[lid] * npix + (size_t)(pl >> 16) * WKA(t.W) + (pl & 0xFFFFu)) * 3;
        dst[0] = HS(0);
        dst[1] = HS(1);
        dst[2] = HS(2);
        have_unit = false;
      }
    }
    // ---- owners waiting on other lanes' samples fold their ring in order ----
    if constexpr (tail) {
      // the ring entries written above, read by other lanes of this wave
      // (wavefront scope: as wf_drain's ring, rtw_wavefront.hip)
      wave_lds_sync();
      if (waiting) {
        uint32_t rdy = TL_READY[lid];
        const double* rb = WKA(ring) + (size_t)(blockIdx.x * kWorldBlock + threadIdx.x) * kTailWin * 3;
        double sx = HS(0), sy = HS(1), sz = HS(2);
        while (L.s != L.s_end && ((rdy >> (L.s % kTailWin)) & 1u)) {
          const uint32_t j = L.s % kTailWin;
          sx += rb[3 * j];
          sy += rb[3 * j + 1];
          sz += rb[3 * j + 2];
          rdy &= ~(1u << j);
          L.s++;
        }
        HS(0) = sx, HS(1) = sy, HS(2) = sz;
        TL_READY[lid] = rdy;
        if (L.s == L.s_end) {
          const uint32_t npix = WKA(t.row_count) * WKA(t.W);
          const uint32_t pl = TL_PXLY[lid];
          double* dst = WKA(t.partial) + ((size_t)TL_C[lid] * npix + (size_t)(pl >> 16) * WKA(t.W) + (pl & 0xFFFFu)) * 3;
          dst[0] = sx;
          dst[1] = sy;
          dst[2] = sz;
          have_unit = false;
          waiting = false;
        }
      }
    }
    return 0;
  };
  for (;;) {
    if (body(std::false_type{}) == 1) break;
    if (WKA(tail_deal) != 0u && __any(done)) {
      while (body(std::true_type{}) != 1) {
      }
      break;
    }
  }
#undef TL_HI
#undef TL_READY
#undef TL_PXLY
#undef TL_LIST
#undef TL_OWN
#undef TL_C
#undef HS
  if constexpr (MODE == 2) {
    WSTAMP(0)
    if (lid == 0)
      for (int i = 0; i < 5; ++i) atomicAdd(A.counts + 8 + i, (unsigned long long)st.ph[i]);
  }
  if constexpr (MODE == 1) {
    atomicAdd(A.counts + 0, n_samples);
    atomicAdd(A.counts + 1, n_segments);
    atomicAdd(A.counts + 2, n_visits);
    atomicAdd(A.counts + 3, n_tests);
    if (lid == 0) atomicAdd(A.counts + 4, n_iters);
    if ((FEAT & kFeatLane) && lid == 0) {
      atomicAdd(A.counts + 5, n_wi);
      atomicAdd(A.counts + 6, n_wl);
    }
  }
}

size_t world_lds_bytes(uint32_t, int fs) {
  return (size_t)((fs & kFeatLane) ? kLaneWaveWords : kBvhStack) * (kWorldBlock / 64) * sizeof(uint32_t);
}

template <int OCC, int FEAT>
static void launch_occ(const WorldArgs& a, uint32_t grid, size_t lds, hipStream_t s, int mode) {
#ifdef RTW_MEASURE
  if (mode == 2) {
    hipLaunchKernelGGL((world_kernel<2, OCC, FEAT>), dim3(grid), dim3(kWorldBlock), lds, s, a);
    return;
  }
#endif
  if (mode == 1)
    hipLaunchKernelGGL((world_kernel<1, OCC, FEAT>), dim3(grid), dim3(kWorldBlock), lds, s, a);
  else
    hipLaunchKernelGGL((world_kernel<0, OCC, FEAT>), dim3(grid), dim3(kWorldBlock), lds, s, a);
}
template <int FEAT>
static void launch_feat(const WorldArgs& a, uint32_t grid, size_t lds, hipStream_t s, int mode, int occ) {
#ifdef RTW_WORLD_ISA_QUICK  // (ISA inspection of the globe's kernel only: tools/isa_world.sh)
  if constexpr (FEAT == (kFeatImage | kFeatLane | kFeatPacked)) hipLaunchKernelGGL((world_kernel<0, 4, FEAT>), dim3(grid), dim3(kWorldBlock), lds, s, a);
#else
  if (occ >= 4)
    launch_occ<4, FEAT>(a, grid, lds, s, mode);
  else if (occ == 3)
    launch_occ<3, FEAT>(a, grid, lds, s, mode);
  else
    launch_occ<1, FEAT>(a, grid, lds, s, mode);
#endif
}
// Instantiated feature sets: spheres with solid / checker / image textures
// (scenes 1, 2, 4 and configs[4]'s globe), rects + transforms + lights without
// noise / image (the Cornell box, scene 5's light), and everything.
int world_feature_set(uint32_t feat, bool lane, bool packed) {
  if (feat & (uint32_t)kFeatTri) {  // triangles: spheres + triangles without chains (meshes; per lane too), or everything
    if ((feat & ~(uint32_t)(kFeatImage | kFeatTri)) == 0u)
      return kFeatTri | (lane ? (packed ? (kFeatImage | kFeatLane | kFeatPacked) : (kFeatImage | kFeatLane)) : kFeatImage);
    return kFeatAll | kFeatTri;
  }
  if ((feat & ~(uint32_t)kFeatImage) == 0u)
    return lane ? (packed ? (kFeatImage | kFeatLane | kFeatPacked) : (kFeatImage | kFeatLane)) : kFeatImage;
  if ((feat & ~(uint32_t)(kFeatXform | kFeatRect)) == 0u) return kFeatXform | kFeatRect;
  return kFeatAll;
}
hipError_t launch_world(const WorldArgs& a, uint32_t grid, size_t lds, hipStream_t s, int mode, int occ, int fs) {
  if (fs == (kFeatImage | kFeatLane | kFeatPacked))
    launch_feat<kFeatImage | kFeatLane | kFeatPacked>(a, grid, lds, s, mode, occ);
  else if (fs == (kFeatImage | kFeatLane))
    launch_feat<kFeatImage | kFeatLane>(a, grid, lds, s, mode, occ);
  else if (fs == kFeatImage)
    launch_feat<kFeatImage>(a, grid, lds, s, mode, occ);
  else if (fs == (kFeatXform | kFeatRect))
    launch_feat<kFeatXform | kFeatRect>(a, grid, lds, s, mode, occ);
  else if (fs == (kFeatTri | kFeatImage | kFeatLane | kFeatPacked))
    launch_feat<kFeatTri | kFeatImage | kFeatLane | kFeatPacked>(a, grid, lds, s, mode, occ);
  else if (fs == (kFeatTri | kFeatImage | kFeatLane))
    launch_feat<kFeatTri | kFeatImage | kFeatLane>(a, grid, lds, s, mode, occ);
  else if (fs == (kFeatTri | kFeatImage))
    launch_feat<kFeatTri | kFeatImage>(a, grid, lds, s, mode, occ);
  else if (fs == (kFeatTri | kFeatAll))
    launch_feat<kFeatTri | kFeatAll>(a, grid, lds, s, mode, occ);
  else
    launch_feat<kFeatAll>(a, grid, lds, s, mode, occ);
  return hipGetLastError();
}

template <int FEAT>
static int bpc_feat(size_t lds, int occ) {
  int nb = 0;
  hipError_t e;
#ifdef RTW_WORLD_ISA_QUICK
  e = hipSuccess, nb = 1, (void)lds, (void)occ;
#else
  if (occ >= 4)
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, world_kernel<0, 4, FEAT>, kWorldBlock, lds);
  else if (occ == 3)
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, world_kernel<0, 3, FEAT>, kWorldBlock, lds);
  else
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, world_kernel<0, 1, FEAT>, kWorldBlock, lds);
#endif
  return (e == hipSuccess && nb > 0) ? nb : 1;
}
int world_blocks_per_cu(size_t lds, int occ, int fs) {
  if (fs == (kFeatImage | kFeatLane | kFeatPacked)) return bpc_feat<kFeatImage | kFeatLane | kFeatPacked>(lds, occ);
  if (fs == (kFeatImage | kFeatLane)) return bpc_feat<kFeatImage | kFeatLane>(lds, occ);
  if (fs == kFeatImage) return bpc_feat<kFeatImage>(lds, occ);
  if (fs == (kFeatXform | kFeatRect)) return bpc_feat<kFeatXform | kFeatRect>(lds, occ);
  if (fs == (kFeatTri | kFeatImage | kFeatLane | kFeatPacked)) return bpc_feat<kFeatTri | kFeatImage | kFeatLane | kFeatPacked>(lds, occ);
  if (fs == (kFeatTri | kFeatImage | kFeatLane)) return bpc_feat<kFeatTri | kFeatImage | kFeatLane>(lds, occ);
  if (fs == (kFeatTri | kFeatImage)) return bpc_feat<kFeatTri | kFeatImage>(lds, occ);
  if (fs == (kFeatTri | kFeatAll)) return bpc_feat<kFeatTri | kFeatAll>(lds, occ);
  return bpc_feat<kFeatAll>(lds, occ);
}

}  // namespace rtwk
