// kbj_obs_encode.h — the projected-gravity encoding of the observation rows (train.py:1338-1349), ONE definition for the env kernel
// that packs the training rows (kbj_env_task.h task_write_obs) and the deployed actor step that packs its own (kbj_deploy.h): the
// deployed actor sees the arithmetic it was trained on.
#pragma once
#include "kbj_env_core.h"

namespace kbj {

KBJ_DEV void encode_pg(const float* g, float* o) {  // train.py:1338-1349
  float n = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  o[0] = atan2f(g[1], -g[2]); o[1] = atan2f(-g[0], sqrtf(g[1] * g[1] + g[2] * g[2]));
  o[2] = g[0] / n; o[3] = g[1] / n; o[4] = g[2] / n;
}

}  // namespace kbj
