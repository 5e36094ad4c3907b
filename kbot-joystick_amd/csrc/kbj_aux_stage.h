// kbj_aux_stage.h — the staged aux row of the per-mode statistics (kbj_tracking_stats.h, kbj_gait_stats.h). A staging wavefront holds one
// time step of its workgroup's aux rows as coalesced 16-byte pieces in registers (piece i = k * 64 + lane of the step: env i / 18, piece
// i % 18 of that env's row), puts the pieces the kernel reads into LDS, one row per env, and every lane then reads its env's row by aux
// column. The row stride is odd, so one env per lane reads conflict-free.
// Which pieces a kernel fetches, and when, is the kernel's: tracking_stats_kernel loads all 18 in two halves around its evaluation,
// gait_stats_kernel only the 13 it reads, in one go.
//
// `Map` says which pieces are staged:
//   static constexpr int NPIECE;                    staged 16-byte pieces of an aux row
//   static __device__ constexpr int piece(int p);   where piece p (columns 4 p .. 4 p + 3) lives in the staged row, or -1
#pragma once
#include <hip/hip_runtime.h>
#include "kbj.h"

namespace kbj {
namespace {

constexpr int AUX_V4 = KBJ_AUX_SIZE / 4;     // 16-byte pieces per aux row
static_assert(KBJ_AUX_SIZE % 4 == 0, "an aux row is whole 16-byte pieces");

// a staged row, read by aux column
template <class Map> struct StagedRow {
  static constexpr int LD = 4 * Map::NPIECE + 1;     // row stride of the staged image, in words
  const float* p;
  static __device__ constexpr int col(int c) { return 4 * Map::piece(c / 4) + c % 4; }
  __device__ float operator[](int c) const { return p[col(c)]; }
};

// piece i of one time step (i = k * 64 + lane in a lane's k-th register: env i / AUX_V4, piece i % AUX_V4 of its row) into the staged image
// `dst` of that step ([env * LD + column]), if it is staged; npiece: the pieces of the step that exist (envs of the workgroup x AUX_V4)
template <class Map> __device__ inline void stage_piece(float* dst, float4 v, int i, int npiece) {
  const int slot = Map::piece(i % AUX_V4);
  if (i < npiece && slot >= 0) { float* d = dst + (i / AUX_V4) * StagedRow<Map>::LD + 4 * slot; d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }
}

// the mode of a row's command (kbj.h kbj_tracking_stats; the switch list of train.py:752-762)
template <class Row> __device__ inline int cmd_mode(const Row& a) {
  const bool x = a[KBJ_AUX_CMD] != 0.0f, y = a[KBJ_AUX_CMD + 1] != 0.0f, z = a[KBJ_AUX_CMD + 2] != 0.0f;
  bool pose = false;
#pragma unroll
  for (int k = 3; k < KBJ_NCMD; ++k) pose = pose || a[KBJ_AUX_CMD + k] != 0.0f;
  if (!(x || y || z)) return pose ? KBJ_CMODE_STAND_BEND : KBJ_CMODE_STAND;
  if (pose || (int)x + (int)y + (int)z != 1) return KBJ_CMODE_OMNI;
  return x ? KBJ_CMODE_FORWARD : y ? KBJ_CMODE_SIDEWAYS : KBJ_CMODE_ROTATE;
}

}  // namespace
}  // namespace kbj
