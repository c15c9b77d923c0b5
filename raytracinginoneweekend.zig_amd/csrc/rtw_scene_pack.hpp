// rtw_scene_pack.hpp — the cover scene's device tables (rtw_internal.hpp has
// the layout), built on the host as one blob that rtw_scene_create
// (rtw_capi.hip) uploads as it stands.  Host only, no HIP and no environment:
// tests/native/scene_pack_check.cpp builds it with a plain C++ compiler and
// checks the tables against the spheres they were made from.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "rtw_hip.h"

namespace rtwp {

// The blob's tables, in blob order.
enum SceneTable {
  kSph64, kRad64, kMat64, kTg64, kSph32, kRad32, kMat32, kTg32, kMeta, kKind, kPerm,
  kCull, kCullTg, kCcull, kCcullTg, kCclus, kCpos, kCvalid, kSceneTables
};

struct ScenePack {
  std::vector<unsigned char> blob;  // every table, each at a 256-B aligned offset
  size_t off[kSceneTables] = {};    // byte offset of each table in the blob
  // the scalars of rtwk::SceneView (both precisions) and of the scene handle
  uint32_t n = 0, nm = 0, ng = 0;
  uint32_t g_end[3] = {0, 0, 0};  // ends of the static wide, static and moving wide groups
  uint32_t nn = 0, nn_pad = 0, n_sn = 0;
  uint32_t cull_on = 0;
  float cmax = 0.0f, rho = 0.0f;  // bounds over the narrow spheres (SceneView cull_cmax, cull_rho)
  uint32_t n_clusters = 0;
  uint32_t cluster_ok = 0;  // the clustered pretest is usable: clusters exist, cull_on, cmax_all within the limit
  float cmax_all = 0.0f;    // cmax over members and cluster centres
  float rho_c = 0.0f;       // SceneView cull_rho_cl
  uint32_t n_static = 0, n_moving = 0, n_wide = 0;
  std::vector<std::pair<double, double>> groups;  // moving-sphere time groups (t0, t1)
};

// Validates the lists and builds the tables.  Returns RTW_OK, or the status of
// the first failed check with its message in `msg`.
int pack_scene(const rtw_sphere* spheres, uint32_t n, const rtw_material* mats, uint32_t nm, ScenePack& out,
               std::string& msg);

}  // namespace rtwp
