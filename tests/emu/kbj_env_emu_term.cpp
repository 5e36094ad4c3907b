// Host emulation build of the env-step kernel body WITH the terminal critic row (task_step's critic_term; kbj_env_step_terminal on the GPU).
// TEST INFRASTRUCTURE ONLY, beside kbj_env_emu.cpp (which stays as it is and keeps compiling against the defaulted argument): one entry, the
// step of kbj_emu_env_step plus `ct` [N][ld_critic], which may be null (= the step without the feature, for the bit-identity check).
#define KBJ_EMU 1
#include "../../kbot-joystick_amd/csrc/kbj_env_task.h"
#include <cstring>
#include <memory>

using namespace kbj;

extern "C" void kbj_emu_env_step_term(const kbj_model* m, const kbj_config* c, uint32_t seed, float* ep, float* es, const float* action, float* aux_t,
                                      float* an, float* cn, float* xn, float* ct) {
  const PhysConst pc = phys_const(*c, *m);
  const size_t lda = KBJ_LD_OF(KBJ_NOBS_ACTOR + c->extra_obs_actor), ldc = KBJ_LD_OF(KBJ_NOBS_CRITIC + c->extra_obs_critic);
#pragma omp parallel for schedule(static)
  for (int i = 0; i < c->num_envs; ++i) {
    std::unique_ptr<KbjShared> S(new KbjShared());
    std::memset(S.get(), 0, sizeof(KbjShared));
    model_lds_fill(S->mc, *m);
    S->pc = pc;
    std::memcpy(S->ep, ep + (size_t)i * KBJ_EP_SIZE, sizeof(S->ep));
    std::memcpy(S->es, es + (size_t)i * KBJ_ES_SIZE, sizeof(S->es));
    Rng rng{seed, (uint32_t)(c->env_id_offset + i)};
    task_step(*S, *m, *c, S->pc, rng, action + (size_t)i * KBJ_NU, aux_t + (size_t)i * KBJ_AUX_SIZE, an + i * lda, cn + i * ldc, xn + (size_t)i * KBJ_AUX_SIZE,
              nullptr, ct ? ct + i * ldc : nullptr);
    std::memcpy(ep + (size_t)i * KBJ_EP_SIZE, S->ep, sizeof(S->ep));
    std::memcpy(es + (size_t)i * KBJ_ES_SIZE, S->es, sizeof(S->es));
  }
}
