"""GPU tests of the host-side contract around the hot path: bit-exact checkpoint resume (xax-layout ckpt.bin), user-edited reward
table vs the oracle, deterministic validation rollouts, the scalar logger fed by a real run, fail-stop behaviour when a persistent
recurrence times out, the accumulate-per-pass exchange variant, and bench.py's own N-rank launch."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from kbot_joystick_amd.spec import constants, layout as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small(**kw):
    from kbot_joystick_amd.host.task import launch_config
    base = dict(num_envs=64, batch_size=32, hidden_size=64, rollout_length_seconds=0.2, robot="kbot-headless", seed=4, num_passes=1)
    base.update(kw)
    return launch_config(**base)


@pytest.mark.parametrize("mirror", [False, True])
def test_checkpoint_resume_is_bit_identical(tmp_path, mirror):
    """save_checkpoint after iteration 2, load into a FRESH task: the rollout of iteration 3 is BIT-identical in both runs (parameters,
    env rows, reward carries, model carries, pending observation rows all travel through ckpt.bin) and the update agrees to the
    run-to-run noise of the fp32 atomic gradient accumulation (the split-K weight gradients add in arrival order)."""
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    kw = dict(actor_mirror_loss_scale=1.0, critic_mirror_loss_scale=0.01) if mirror else {}
    cfg = _small(num_passes=2, **kw)
    a = HumanoidWalkingTask(cfg)
    for _ in range(2):
        a.train_iteration()
    path = str(tmp_path / "ckpt.bin")
    a.save_checkpoint(path)
    a.train_iteration()
    torch.cuda.synchronize()
    b = HumanoidWalkingTask(cfg)
    b.load_checkpoint(path)
    assert (b.iteration, b.opt_step) == (2, a.opt_step - 4)
    b.train_iteration()
    torch.cuda.synchronize()
    for name in ("actor_obs", "critic_obs", "aux", "action", "logp", "value", "reward", "carry0_actor_hc", "carry0_critic_hc", "carry0_lpf"):
        assert torch.equal(getattr(a.traj, name), getattr(b.traj, name)), name
    for name, tol, cap in (("params", 1e-6, 4 * cfg.learning_rate), ("opt_m", 1e-6, 1e-4), ("opt_v", 1e-8, 1e-6)):
        d = (getattr(a, name) - getattr(b, name)).abs()       # Adam amplifies last-bit gradient noise on near-zero gradients (see above)
        assert float((d > tol).float().mean()) < 1e-3 and float(d.max()) <= cap, name
    assert a.opt_step == b.opt_step
    assert torch.equal(a.carry.actor_hc, b.carry.actor_hc) and torch.equal(a.carry.lpf, b.carry.lpf)
    ea, eb = a.ctx.env_get_state(), b.ctx.env_get_state()
    assert np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1].view(np.uint32), eb[1].view(np.uint32))
    assert np.array_equal(a.ctx.env_get_reward_carry(), b.ctx.env_get_reward_carry())
    # load_task rebuilds the task from the checkpoint's own config member (convert.py:36); load_ckpt(part="model") as convert.py:39
    c = HumanoidWalkingTask.load_task(path)
    assert c.config.hidden_size == cfg.hidden_size and c.iteration == 2
    mv = c.load_ckpt(path, part="model")[0]
    n = c.ctx.actor_param_count()
    flat = np.concatenate([mv.leaves[k].ravel() for k in mv.leaves if k.startswith("actor.")])
    assert flat.size == n and mv.carry_size == 2 * 2 * cfg.hidden_size + 20
    for t in (a, b, c):
        t.ctx.close()


@pytest.mark.parametrize("H,D,mirror", [(192, 3, False), (128, 1, False), (64, 3, True), (384, 2, False)])
def test_task_runs_with_other_depths_and_hidden_sizes(tmp_path, H, D, mirror):
    """The reference's model fields hidden_size / depth (train.py:78-85) through the whole task: iterations run, the checkpoint carries
    depth x (h, c) planes and the exported actor advertises carry_size = depth * 2 * hidden + 20 (convert.py:71)."""
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    from kbot_joystick_amd.host import ckpt
    kw = dict(actor_mirror_loss_scale=1.0, critic_mirror_loss_scale=0.01) if mirror else {}
    t = HumanoidWalkingTask(_small(hidden_size=H, depth=D, num_passes=2, **kw))
    for _ in range(2):
        t.train_iteration()
    assert bool(torch.isfinite(t.metrics).all()) and bool(torch.isfinite(t.params).all())
    assert tuple(t.carry.actor_hc.shape) == (D, 2, 64, H) and float(t.carry.actor_hc.abs().sum()) > 0
    if mirror:
        assert tuple(t.carry.actor_mirror_hc.shape) == (D, 2, 64, H) and float(t.carry.critic_mirror_hc.abs().sum()) > 0
    path = str(tmp_path / "ckpt.bin")
    t.save_checkpoint(path)
    flat = ckpt.load_ckpt(path, "model", hidden_size=H, depth=D)
    assert flat.shape[0] == sum(L.param_count(H, D)) and np.array_equal(flat, t.params.cpu().numpy())
    mv = t.load_ckpt(path, part="model")[0]
    assert mv.depth == D and len(mv.actor.rnns) == D and mv.carry_size == D * 2 * H + 20
    t.ctx.close()


def test_edited_reward_table_matches_oracle(model):
    """f3: scales / error scales are data (kbj_config), not kernel literals: a user-edited stack gives the oracle's numbers."""
    import torch
    from kbot_joystick_amd.host import binding as B
    from oracle import oracle as O
    N, T = 64, 12
    rng = np.random.default_rng(3)
    over = dict(rew_linvel_err=0.35, rew_rollpitch_err=0.05, rew_standard_height=0.75, rew_grace_period=0.1, rew_touchdown_penalty=0.2, rew_torque_err=2.0)
    cfg = L.default_config(num_envs=N, batch_size=N, **over)
    for i, s in enumerate((0.3, 0.0, 0.1, 0.4, 0.0, 0.2, 0.3, 0.7, 0.05, 0.2, 0.0, 0.6)):
        cfg.reward_scale[i] = s
    base = L.default_config(num_envs=N, batch_size=N)
    # a plausible trajectory: roll the oracle env for T steps with random actions
    o = O.Oracle(model, cfg, seed=2, precision="f32")
    _, _, x = o.reset_all()
    aux = np.zeros((T + 1, N, L.AUX["SIZE"]), np.float32)
    aux[0] = x
    from tests import helpers as H
    for t in range(T):
        _, _, aux[t + 1] = o.step(H.random_actions(model, rng, N, 0.5), aux[t])
    r_o, c_o = o.rewards(aux[:T])
    r_b, _ = O.Oracle(model, base, seed=2, precision="f32").rewards(aux[:T])
    assert np.abs(r_o - r_b).max() > 0.05                                            # the edit really changes the reward
    ctx = B.Context(model, cfg, 0, torch.cuda.current_stream().cuda_stream)
    rew = torch.zeros(T, N, device="cuda:0"); comps = torch.zeros(T, N, L.NREW, device="cuda:0")
    a, c, xx = (torch.zeros(N, d, device="cuda:0") for d in (L.LD_ACTOR, L.LD_CRITIC, L.AUX["SIZE"]))
    ctx.env_reset_all(2, a, c, xx)                                                    # initialises the reward carries as the oracle's
    ctx.rewards(torch.from_numpy(aux[:T].copy()).cuda(), T, rew, comps)
    ctx.synchronize()
    assert np.abs(comps.cpu().numpy() - c_o).max() < 2e-4 and np.abs(rew.cpu().numpy() - r_o).max() < 2e-4
    ctx.close()


def test_python_reward_terms_on_the_trajectory_view():
    """f3: a user-written term in ksim's Reward protocol runs on the stored trajectory (torch, GPU) and is added before GAE. The view's
    semantics are checked by restating two built-in terms in Python against the kernel's own components."""
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    from kbot_joystick_amd.host.traj_view import TrajectoryView

    class Alive:                                                     # stateless (train.py:161-165 protocol)
        scale = 0.25
        def get_reward(self, traj):
            return (traj.done == 0).float()

    class StepsSinceDone:                                            # stateful (train.py:135-154 protocol): carry = steps since the last done
        scale = 0.01
        def initial_carry(self, n, device):
            return torch.zeros(n, device=device)
        def get_reward_stateful(self, traj, carry):
            out = torch.empty(traj.T, traj.N, device=carry.device)
            for t in range(traj.T):
                carry = torch.where(traj.done[t] != 0, torch.zeros_like(carry), carry + 1)
                out[t] = carry
            return out, carry

    cfg = _small(log_reward_components=True)
    plain = HumanoidWalkingTask(cfg)
    task = HumanoidWalkingTask(cfg, extra_rewards={"alive": Alive(), "since_done": StepsSinceDone()})
    plain.rollout(); task.rollout()
    torch.cuda.synchronize()
    view = TrajectoryView(task.traj, task.T)
    want = plain.traj.reward + 0.25 * (view.done == 0).float()
    carry, extra = torch.zeros(task.N, device="cuda"), torch.zeros_like(want)
    for t in range(task.T):
        carry = torch.where(view.done[t] != 0, torch.zeros_like(carry), carry + 1); extra[t] = carry
    assert torch.allclose(task.traj.reward, want + 0.01 * extra, atol=1e-6)
    assert set(task.extra_reward_means) == {"alive", "since_done"}
    # the view against the kernel: angvel (train.py:301-306) and torque (train.py:503-506) restated in torch
    k = task.kcfg
    comps = task.traj.comps
    angvel = torch.exp(-(view.base_qvel[..., 5] - view.command[..., 2]).abs() / k.rew_angvel_err)
    assert torch.allclose(angvel, comps[..., constants.REWARD_NAMES.index("angvel")], atol=1e-5)
    zc = view.command[..., :3].norm(dim=-1) < 1e-3
    torque = torch.where(zc, torch.exp(-view.ctrl.abs() / k.rew_torque_err).mean(-1), torch.ones_like(view.base_z))
    assert torch.allclose(torque, comps[..., constants.REWARD_NAMES.index("torque")], atol=1e-5)
    task.update()                                                    # GAE and the update run on the augmented reward
    torch.cuda.synchronize()
    assert torch.isfinite(task.params).all()
    plain.ctx.close(); task.ctx.close()


def test_validation_is_deterministic_and_leaves_training_untouched():
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    task = HumanoidWalkingTask(_small(log_reward_components=True))
    task.train_iteration()
    p0, es0 = task.params.clone(), task.ctx.env_get_state()[1].copy()
    v1 = task.validate(num_envs=32, seconds=1.0)
    v2 = task.validate(num_envs=32, seconds=1.0)
    assert v1 == v2 and all(np.isfinite(x) for x in v1.values())                     # argmax actions, fixed seed: bit-reproducible
    # the plain validation is ONE kbj_rollout call in argmax mode (kbj_set_rollout_argmax); the step-by-step loop that view() and the user-term
    # paths run gives the same numbers, bit for bit
    assert task.validate(num_envs=32, seconds=1.0, _stepwise=True) == v1
    assert set(f"valid/reward/{n}" for n in constants.REWARD_NAMES) <= set(v1)
    assert torch.equal(p0, task.params) and np.array_equal(es0.view(np.uint32), task.ctx.env_get_state()[1].view(np.uint32))
    sc = task.scalars()
    assert abs(sum(constants.REWARD_SCALES[i] * sc[f"reward/{n}"] for i, n in enumerate(constants.REWARD_NAMES)) - sc["train/reward_per_step"]) < 1e-4
    task.ctx.close()


def test_launch_writes_logs_and_checkpoint(tmp_path):
    from kbot_joystick_amd.host import ckpt, scalars as S
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    cfg = _small(valid_every_n_steps=2, render_length_seconds=0.4, log_reward_components=True, save_every_n_seconds=0.0001)
    run = str(tmp_path / "humanoid_walking_task" / "run_0")
    task = HumanoidWalkingTask.launch(cfg, num_iterations=3, run_dir=run, quiet=True)
    ev = S.read_event_file(glob.glob(os.path.join(run, "logs", "events.out.tfevents.*"))[0])
    assert [s for s, _ in ev] == [1, 2, 3] and "valid/reward_per_step" in ev[1][1] and "valid/reward_per_step" not in ev[0][1]
    assert {"train/loss", "train/reward_per_step", "reward/feet_airtime", "perf/env_steps_per_s"} <= set(ev[0][1])
    z = ckpt.load_ckpt(os.path.join(run, "checkpoints", "ckpt.bin"))                   # convert.sh:4 path convention
    assert z["state"]["num_steps"] == 3 and np.array_equal(z["model"], task.params.cpu().numpy())
    task.ctx.close()


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_recurrence_timeout_is_fail_stop(monkeypatch, which):
    """Fault injection: the first forward (or backward: lstm_seq_bwd16_kernel, hidden 128 = two partners per row group) recurrence of the
    update is launched with one workgroup missing, so its partners' bounded spins expire. The gradient is poisoned on the device, the
    optimizer step is skipped (parameters and moments unchanged), the error surfaces as KbjError at the iteration's synchronisation point,
    and the context stays usable and destroyable."""
    import torch
    from kbot_joystick_amd.host import binding as B
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    var = "KBJ_DEBUG_DROP_SEQ_WG" if which == "forward" else "KBJ_DEBUG_DROP_SEQ_BWD_WG"
    monkeypatch.setenv(var, "1")
    task = HumanoidWalkingTask(_small(num_envs=64, batch_size=64, hidden_size=64 if which == "forward" else 128))
    monkeypatch.delenv(var)
    p0 = task.params.clone()
    import time
    t0 = time.perf_counter()
    with pytest.raises(B.KbjError, match="timed out"):
        task.train_iteration()
    torch.cuda.synchronize()
    # time to fail: the waits are bounded in WALL-CLOCK time (20 ms under fault injection, 2 s by default) and every launch behind the first
    # failure aborts at entry, so the whole iteration - one timed-out hand-off, then ~10 aborted calls - is over in well under the default bound
    assert time.perf_counter() - t0 < 5.0, time.perf_counter() - t0
    assert torch.equal(p0, task.params) and float(task.opt_m.abs().max()) == 0.0      # the step was a no-op on the device
    task.train_iteration()                                                            # the injected fault is spent: the context still works
    torch.cuda.synchronize()
    assert torch.isfinite(task.params).all() and not torch.equal(p0, task.params)
    task.ctx.close()


def test_per_pass_accumulate_variant_matches_manual_accumulation():
    """KBJ_ALLREDUCE=per_pass: one optimizer step per pass on the mean of the pass's minibatch gradients."""
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    cfg = _small(num_envs=128, batch_size=32, num_passes=2, allreduce="per_pass")
    task = HumanoidWalkingTask(cfg)
    task.rollout()
    ref = HumanoidWalkingTask(_small(num_envs=128, batch_size=32, num_passes=2))
    for name in ("actor_obs", "critic_obs", "aux", "action", "logp", "value", "reward", "carry0_actor_hc", "carry0_critic_hc", "carry0_lpf"):
        getattr(ref.traj, name).copy_(getattr(task.traj, name))
    task.update()
    torch.cuda.synchronize()
    assert task.opt_step == 2
    # manual restatement on the second task: same permutations, accumulate 4 gradients, one AdamW step with scale 1/4
    ref.ctx.gae(ref.traj.c, ref.traj.adv, ref.traj.target)
    for p in range(2):
        g = torch.Generator(device="cpu"); g.manual_seed((cfg.seed * 1000003 + 0 * 97 + p) & 0x7FFFFFFF)
        perm = torch.randperm(128, generator=g).int().cuda()
        acc = torch.zeros_like(ref.params)
        for mb in range(4):
            ref.ctx.ppo_grad(ref.params, ref.traj.c, perm[32 * mb:32 * mb + 32].contiguous(), 32, ref.traj.adv, ref.traj.target, ref.grad, ref.metrics)
            acc += ref.grad
        ref.ctx.adamw_step(ref.params, ref.opt_m, ref.opt_v, acc, p + 1, 0.25)
    torch.cuda.synchronize()
    # the split-K weight gradients add in arrival order (fp32 atomics), and Adam's m / sqrt(v) turns a last-bit difference of a
    # near-zero gradient into a step of up to the learning rate: compare in distribution, bound the extreme by two steps
    d = (task.params - ref.params).abs()
    assert float((d > 1e-6).float().mean()) < 1e-3 and float(d.max()) <= 2 * 2 * cfg.learning_rate
    task.ctx.close(); ref.ctx.close()


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` (no torchrun around it) starts two ranks itself before touching the GPU. On this one-GPU box the
    ranks share GPU 0 and gloo carries the gradient (RCCL refuses two ranks on one device); the 8-GPU job differs only in
    --backend nccl and one GPU per rank."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu", "--envs-per-gpu", "512",
                          "--hidden", "64", "--steps", "1", "--warmup", "1", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["n_gpus"] == 2 and rec["value"] > 0 and rec["config"]["envs_per_gpu"] == 512 and rec["scaling"] == "weak"
    assert abs(rec["value"] - 2 * 512 * 100 / (rec["ms_per_step"] * 1e-3)) < 1e-3 * rec["value"]
    # a mismatch between --gpus and the launcher's world size is an error, not a silent pass
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, timeout=120,
                         env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert bad.returncode != 0 and "does not match WORLD_SIZE" in (bad.stderr + bad.stdout)


def test_bench_line_carries_the_child_process_legs():
    """`bench.py --gpus 1 --full` (at a small size): after the headline is measured the two NON-headline legs run in child
    processes - `variant_gemm_bf16x3` and `train_loop` (launch() with logging, validation rollouts and background checkpoints) - and a leg that
    dies costs its own object, never the line."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs-per-gpu", "512", "--hidden", "64", "--steps", "2", "--warmup", "1",
           "--full", "--no-cpu-baseline", "--loop-iterations", "30"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                        # ONE JSON line, whatever the children print
    rec = json.loads(lines[0])
    assert rec["value"] > 0 and rec["dtype"] == "f32" and rec["variant"].startswith("headline")
    v, tl = rec["variant_gemm_bf16x3"], rec["train_loop"]
    assert v["NOT_THE_HEADLINE"] and v["value"] > 0 and "child" in v["process"]
    assert tl["value"] > 0 and tl["iterations"] == 30 and tl["validations"] == 1 and tl["vs_headline"] > 0 and tl["checkpoint_bytes"] > 0
    # a leg that fails (here: an impossible loop length is fine, so break the child through its environment) leaves an error in ITS object only
    bad = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(env, KBJ_LIB_NAME="libkbj_does_not_exist.so"))
    assert bad.returncode != 0                                     # without the library nothing runs at all: the product path fails loudly
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--leg", "variant", "--gpus", "1", "--envs-per-gpu", "512", "--hidden", "64", "--steps", "1",
                          "--warmup", "1"], capture_output=True, text=True, timeout=600, env=env)
    assert one.returncode == 0 and json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])["name"] == "gemm_bf16x3"


def test_bench_forced_collective_on_one_gpu():
    """`bench.py --gpus 1 --force-collective --full`: the RCCL leg (backend nccl, world size 1, gradient all-reduce forced) timed beside the run
    without a process group and the overlapped exchange, in one process; the rank count of the line comes from the process group and an
    all-reduce of ones, not from the environment; the all-reduce time comes from --full's instrumented iteration."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29547")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-collective", "--full", "--envs-per-gpu", "1024", "--hidden", "64",
                          "--steps", "2", "--warmup", "1", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    fc = rec["forced_collective"]
    assert rec["rccl_ranks"] == 1 and rec["rccl_ranks_counted_by_allreduce"] == 1 and rec["collective_backend"] == "nccl"
    assert rec["allreduce_calls_per_iteration"] == 3 * (1024 // 512) and rec["allreduce_ms_per_iteration"] > 0
    for k in ("ms_per_step_no_process_group", "ms_per_step_forced_allreduce", "ms_per_step_forced_allreduce_overlapped"):
        assert fc[k] > 0
    assert abs(rec["ms_per_step"] - fc["ms_per_step_forced_allreduce"]) < 1e-6
    assert rec["rank_ms_per_step"]["min"] <= rec["rank_ms_per_step"]["max"]


def test_plain_bench_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` without --full: one JSON line with the headline fields and none of what needs
    runs of its own (roofline, all-reduce timing, CPU baseline, child legs: null); DIR holds the last timed step's outputs as float32 .npy
    files, 64 MB at most. The headline's update reduces in fixed order, so two runs with the same arguments compute the same: after a
    warm-up and two timed iterations every array is bit-identical (the logged metrics, still summed with atomics, to rounding)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs-per-gpu", "512", "--hidden", "64", "--steps", "2",
                              "--warmup", "1", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        rec = json.loads(lines[0])
        assert rec["value"] > 0 and rec["unit"] == "env-steps/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
        assert rec["steps"] == 2 and rec["full"] is False and abs(rec["value"] - 512 * 100 / (rec["ms_per_step"] * 1e-3)) < 1e-3 * rec["value"]
        assert rec["config"]["deterministic_update"] is True
        for k in ("roofline", "roofline_secondary", "hbm_whole_path", "allreduce_ms_per_iteration", "cpu_baseline", "variant_gemm_bf16x3", "train_loop"):
            assert rec[k] is None, k
        files = sorted(glob.glob(str(d / "*.npy")))
        assert sum(os.path.getsize(f) for f in files) <= 64e6
        arrs = {os.path.basename(f)[:-4]: np.load(f) for f in files}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
        dumps.append(arrs)
    a, b = dumps
    assert set(a) == set(b) >= {"params", "metrics", "reward", "done", "action", "actor_obs", "critic_obs"}
    assert a["reward"].shape == (100, 512) and a["action"].shape == (100, 512, L.NU)
    for k in sorted(set(a) - {"metrics"}):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert np.allclose(a["metrics"], b["metrics"], rtol=1e-5, atol=1e-7)


def test_python_termination_and_observation_terms():
    """f3: user-written Termination / Observation terms in the reference's protocol (train.py:817, 635-707) on the post-step StepView.
    The reference's own TerrainBadZTermination (train.py:817-823) restated in Python, with the kernel's built-in bad-z term switched off,
    must give the stock run's DONE column, env rows, actions and actor observations BIT FOR BIT - the env is reset through
    kbj_env_reset_where as the step kernel resets an env its own terminations finish. (The critic's composite-inertia entries of a reset
    row may differ in the last bit: the reset code is compiled into two kernels and hipcc contracts its fused multiply-adds differently;
    they are derived from the state, not part of it, so the env trajectory is unaffected - the values follow to 1e-5.)"""
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask

    class TerrainBadZ:                      # train.py:817-823
        unhealthy_z = 0.4

        def __call__(self, state, curriculum_level):
            height = state.base_z - torch.minimum(state.left_foot_z, state.right_foot_z)
            return torch.where(height < self.unhealthy_z, -1, 0)

    class BaseHeight:                       # train.py:706-707 (xpos[1, 2:])
        def observe(self, state, curriculum_level, rng):
            return state.base_height[:, None]

    kw = dict(num_envs=256, batch_size=64, rollout_length_seconds=1.0)
    stock = HumanoidWalkingTask(_small(**kw))
    user = HumanoidWalkingTask(_small(termination_params={"bad_z": {"unhealthy_z": float("-inf")}}, **kw),
                               extra_terminations={"bad_z": TerrainBadZ()}, extra_observations={"base_height": BaseHeight()})
    assert user.kcfg.unhealthy_z < -1e30 and user.get_terminations()["bad_z"].params["unhealthy_z"] < -1e30
    fails = 0
    for it in range(3):
        stock.rollout(); user.rollout()
        torch.cuda.synchronize()
        for name in ("aux", "actor_obs", "action", "logp", "reward"):          # aux holds the DONE column
            assert torch.equal(getattr(stock.traj, name), getattr(user.traj, name)), (it, name)
        assert float((stock.traj.critic_obs - user.traj.critic_obs).abs().max()) < 1e-6
        assert float((stock.traj.value - user.traj.value).abs().max()) < 1e-5
        fails += int((stock.traj.done < 0).sum())
        stock.iteration += 1; user.iteration += 1
    assert fails > 20                                                   # the random-init policy falls: the user term did fire (and reset) often
    es, eu = stock.ctx.env_get_state(), user.ctx.env_get_state()
    assert np.array_equal(es[0], eu[0]) and np.array_equal(es[1].view(np.uint32), eu[1].view(np.uint32))
    assert torch.equal(stock.carry.actor_hc, user.carry.actor_hc) and float((stock.carry.critic_hc - user.carry.critic_hc).abs().max()) < 1e-5
    # the user observation is the critic row's base-height entry of every step (row t + 1 = the state after step t)
    bh = user.extra_obs_buffers["base_height"]
    assert bh.shape == (user.T + 1, 256, 1) and torch.equal(bh[1:, :, 0], user.traj.critic_obs[1:, :, L.OBS["HEIGHT"][0]])
    # a user term that never fires leaves the run identical to the fused kbj_rollout; a full training iteration runs with both kinds of terms
    user.train_iteration()
    torch.cuda.synchronize()
    assert torch.isfinite(user.params).all()
    with pytest.raises(KeyError):
        _small(termination_params={"bad_z": {"nope": 1.0}}).to_kbj(64)
    stock.ctx.close(); user.ctx.close()
    # with record_state the term can be the reference's body as written (train.py:817-823: `state.xpos[self.base_idx, 2]` per env), evaluated per
    # env under torch.vmap: the same DONE column as the kernel's own bad-z termination
    from kbot_joystick_amd.host.traj_view import per_env_state

    class TerrainBadZTermination:
        def __init__(self, base_idx, foot_left_idx, foot_right_idx, unhealthy_z):
            self.base_idx, self.foot_left_idx, self.foot_right_idx, self.unhealthy_z = base_idx, foot_left_idx, foot_right_idx, unhealthy_z

        def _one(self, state, curriculum_level):
            base_z = state.xpos[self.base_idx, 2]
            left_foot_z = state.xpos[self.foot_left_idx, 2]
            right_foot_z = state.xpos[self.foot_right_idx, 2]
            height = base_z - torch.minimum(left_foot_z, right_foot_z)
            return torch.where(height < self.unhealthy_z, -1, 0)

        def __call__(self, state, curriculum_level):
            return per_env_state(self._one)(state, curriculum_level)
    stock2 = HumanoidWalkingTask(_small(**kw))
    mb = stock2.model_blob
    ref = HumanoidWalkingTask(_small(termination_params={"bad_z": {"unhealthy_z": float("-inf")}}, record_state=True, **kw),
                              extra_terminations={"bad_z": TerrainBadZTermination(int(mb.base_body), int(mb.lfoot_body), int(mb.rfoot_body), 0.4)})
    for it in range(2):
        stock2.rollout(); ref.rollout()
        torch.cuda.synchronize()
        assert torch.equal(stock2.traj.aux, ref.traj.aux) and torch.equal(stock2.traj.action, ref.traj.action), it
        stock2.iteration += 1; ref.iteration += 1
    assert int((ref.traj.done < 0).sum()) > 5
    with pytest.raises(ValueError, match="record_state"):
        from kbot_joystick_amd.host.traj_view import StepView
        StepView(stock2.traj.aux[0], stock2.traj.actor_obs[1], stock2.traj.critic_obs[1], stock2.traj.aux[1], mb).xpos
    stock2.close(); ref.close()


def test_python_command_term():
    """f3: a user-written Command term in the reference's protocol (train.py:724 initial_command, :768 __call__) replaces the built-in
    sampler through kbj_env_set_command. A term that always answers one fixed command must reproduce the library's own fixed-command
    mode (BASELINE configs[1]) BIT FOR BIT; a term that ramps the forward speed with the episode time must show up in the env state,
    the observation rows of both networks, the record the rewards read, and the zero-command flag."""
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask

    class Fixed:
        def __init__(self, v):
            self.v = torch.tensor(list(v) + [0.0] * (L.NCMD - len(v)), device="cuda")

        def initial_command(self, state, curriculum_level, rng):
            return self.v.expand(state.N, L.NCMD)

        def __call__(self, prev_command, state, curriculum_level, rng):
            return prev_command

    class Ramp:                                         # starts standing (zero command), then +0.05 m/s forward per control step
        def initial_command(self, state, curriculum_level, rng):
            return torch.zeros(state.N, L.NCMD, device="cuda")

        def __call__(self, prev_command, state, curriculum_level, rng):
            out = prev_command.clone()
            out[:, 0] = prev_command[:, 0] + 0.05
            out[:, 6] = torch.rand(state.N, device="cuda", generator=rng) * 0.1     # an arm command drawn from the step's generator
            return out

    kw = dict(num_envs=128, batch_size=64, rollout_length_seconds=0.6)
    stock = HumanoidWalkingTask(_small(fixed_command=(0.7, 0.0, 0.2), **kw))
    user = HumanoidWalkingTask(_small(**kw), command=Fixed((0.7, 0.0, 0.2)))
    assert user.kcfg.command_mode == 1
    for it in range(2):
        stock.rollout(); user.rollout()
        torch.cuda.synchronize()
        for name in ("aux", "actor_obs", "critic_obs", "action", "logp", "value", "reward"):
            assert torch.equal(getattr(stock.traj, name), getattr(user.traj, name)), (it, name)
        stock.iteration += 1; user.iteration += 1
    es, eu = stock.ctx.env_get_state(), user.ctx.env_get_state()
    assert np.array_equal(es[1].view(np.uint32), eu[1].view(np.uint32))
    stock.ctx.close(); user.ctx.close()

    ramp = HumanoidWalkingTask(_small(**kw), command=Ramp())
    twin = HumanoidWalkingTask(_small(**kw), command=Ramp())
    ramp.rollout(); twin.rollout()
    torch.cuda.synchronize()
    assert torch.equal(ramp.traj.aux, twin.traj.aux) and torch.equal(ramp.traj.reward, twin.traj.reward)      # the step generator is seeded
    T, tr = ramp.T, ramp.traj
    C, A, O = L.AUX["CMD"], L.AUX, L.OBS
    done = tr.aux[:T, :, A["DONE"]] != 0
    vx = tr.aux[:, :, C]
    assert torch.all(vx[0] == 0)
    expect = torch.where(done, torch.zeros_like(vx[1:]), vx[:-1] + 0.05)            # restart at zero after a reset, else the ramp
    assert torch.equal(vx[1:], expect)
    assert float(vx.max()) >= 0.05 * 10
    assert torch.equal(tr.actor_obs[:, :, O["CMD"][0]:O["CMD"][0] + L.NCMD], tr.aux[:, :, C:C + L.NCMD])
    assert torch.equal(tr.critic_obs[:, :, O["CMD"][0]:O["CMD"][0] + L.NCMD], tr.aux[:, :, C:C + L.NCMD])
    zero = (tr.aux[:, :, C:C + 3].norm(dim=-1) < 1e-3).float()
    assert torch.equal(tr.actor_obs[:, :, O["ZEROCMD"][0]], zero) and torch.equal(tr.critic_obs[:, :, O["ZEROCMD"][0]], zero)
    arm = tr.aux[1:, :, C + 6][~done]
    assert float(arm.min()) >= 0 and float(arm.max()) <= 0.1 and float(arm.std()) > 0.01
    _, es = ramp.ctx.env_get_state()
    assert np.array_equal(es[:, L.ES["CMD"]:L.ES["CMD"] + L.NCMD], tr.aux[T, :, C:C + L.NCMD].cpu().numpy())
    ramp.train_iteration()
    torch.cuda.synchronize()
    assert torch.isfinite(ramp.params).all()
    # the deterministic validation rollout is driven by the same term (its own env set and context)
    v = ramp.validate(num_envs=64, seconds=0.4)
    vtr = ramp._valid[3]
    vdone = vtr.aux[:20, :, A["DONE"]] != 0
    vvx = vtr.aux[:21, :, C]
    assert torch.all(vvx[0] == 0) and torch.equal(vvx[1:], torch.where(vdone, torch.zeros_like(vvx[1:]), vvx[:-1] + 0.05))
    assert np.isfinite(v["valid/reward_per_step"])
    ramp.ctx.close(); twin.ctx.close()


@pytest.mark.parametrize("H,mirror", [(96, False), (160, True), (300, True)])
def test_free_hidden_size_end_to_end(tmp_path, H, mirror):
    """hidden_size is an unconstrained field of the reference's config (train.py:78-81). A hidden size between the kernels' 64-unit steps
    runs zero padded behind the ABI; parameters, carries, gradients and checkpoints keep the CALLER's layout. Checks on a whole task:
    parameter count = the formula for H; the step-by-step rollout (kbj_policy_step / kbj_carry_reset, one boundary conversion per call)
    equals the fused kbj_rollout bit for bit; deterministic training is reproducible and resumes bit-identically from a checkpoint;
    the exported actor carries H-wide leaves."""
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    kw = dict(actor_mirror_loss_scale=1.0, critic_mirror_loss_scale=0.01) if mirror else {}
    cfg = _small(hidden_size=H, deterministic=True, num_passes=2, **kw)
    a = HumanoidWalkingTask(cfg)
    pa, pc = L.param_count(H)
    assert a.P == pa + pc and a.ctx.actor_param_count() == pa and a.carry.actor_hc.shape == (2, 2, 64, H)
    never = lambda state, level: torch.zeros(state.N, device="cuda")
    s = HumanoidWalkingTask(cfg, extra_terminations={"never": never})
    a.rollout(); s.rollout()
    torch.cuda.synchronize()
    for name in ("aux", "actor_obs", "critic_obs", "action", "logp", "value", "reward", "carry0_actor_hc", "carry0_critic_hc"):
        assert torch.equal(getattr(a.traj, name), getattr(s.traj, name)), name
    assert torch.equal(a.carry.actor_hc, s.carry.actor_hc) and torch.equal(a.carry.critic_hc, s.carry.critic_hc)
    assert float(a.carry.actor_hc.abs().max()) > 0.01
    a.update(); s.update()
    a.iteration += 1; s.iteration += 1
    torch.cuda.synchronize()
    assert torch.equal(a.params, s.params) and torch.isfinite(a.params).all() and float(a.grad.abs().max()) > 0
    # on-policy re-evaluation of the stored trajectory with the pre-update parameters is covered by test_gpu_switches; here: resume
    path = str(tmp_path / "ckpt.bin")
    a.save_checkpoint(path)
    a.train_iteration()
    b = HumanoidWalkingTask.load_task(path)
    assert b.config.hidden_size == H
    b.train_iteration()
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params) and torch.equal(a.traj.value, b.traj.value) and torch.equal(a.carry.critic_hc, b.carry.critic_hc)
    mv = b.load_ckpt(path, part="model")[0]
    assert mv.leaves["actor.rnns.0.weight_hh"].shape == (4 * H, H) and mv.carry_size == 2 * 2 * H + 20
    for t in (a, s, b):
        t.ctx.close()


def test_user_observation_routed_into_the_networks(tmp_path):
    """f3: a user-written Observation term (train.py:635-707 protocol) that is a NETWORK INPUT, the reference user's edit of run_actor /
    run_critic (train.py:1351-1433): `extra_observations={name: (term, "both")}` with config.extra_actor_obs / extra_critic_obs floats reserved
    behind the reference's 65 / 475 columns. The rows the networks read carry the term's outputs, the input projections are wider, training
    runs, a checkpoint round-trips (load_task rebuilds the widened model) and validation feeds the term to the policy as well."""
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config
    from kbot_joystick_amd.host import ckpt as ckpt_io

    class FootHeights:                       # 3 floats per env: both feet's height above the lower one + base height
        def observe(self, state, curriculum_level, rng):
            low = torch.minimum(state.left_foot_z, state.right_foot_z)
            return torch.stack([state.left_foot_z - low, state.right_foot_z - low, state.base_height], dim=1)

    cfg = launch_config(num_envs=128, batch_size=64, hidden_size=64, rollout_length_seconds=0.2, robot="kbot-headless", seed=4,
                        extra_actor_obs=3, extra_critic_obs=3)
    with pytest.raises(ValueError, match="routed"):
        HumanoidWalkingTask(cfg)                                              # reserved inputs nobody fills
    task = HumanoidWalkingTask(cfg, extra_observations={"foot_heights": (FootHeights(), "both")})
    assert (task.nobs_actor, task.nobs_critic, task.ld_actor, task.ld_critic) == (68, 478, 68, 480)
    assert task.traj.actor_obs.shape[-1] == 68 and task.traj.critic_obs.shape[-1] == 480
    mv = task.load_ckpt  # noqa: F841 (exists)
    task.train_iteration()
    T = task.T
    fh = task.extra_obs_buffers["foot_heights"]
    for t in (0, 1, T):
        assert torch.equal(task.traj.actor_obs[t][:, 65:68], fh[t]) and torch.equal(task.traj.critic_obs[t][:, 475:478], fh[t])
        assert float(task.traj.critic_obs[t][:, 478:].abs().max()) == 0.0      # the pad stays zero
    assert float(fh.abs().max()) > 0.1 and torch.isfinite(task.params).all() and torch.isfinite(task.metrics).all()
    # the term equals the kernel's own base-height observation (critic column 474) where both exist
    assert torch.allclose(fh[1][:, 2], task.traj.critic_obs[1][:, 474])
    path = str(tmp_path / "ckpt.bin")
    task.save_checkpoint(path)
    z = ckpt_io.load_ckpt(path)
    assert z["config"]["extra_actor_obs"] == 3 and z["model"].size == task.P
    mvw = task.load_ckpt(path)[0]
    assert mvw.actor.input_proj.weight.shape == (64, 68) and mvw.critic.input_proj.weight.shape == (64, 478)
    with pytest.raises(ValueError, match="routed"):
        HumanoidWalkingTask.load_task(path)                                   # the config alone cannot know the user's term ...
    task2 = HumanoidWalkingTask(cfg, extra_observations={"foot_heights": (FootHeights(), "both")})
    task2.load_checkpoint(path)                                               # ... the user passes it again, as in the reference
    task.train_iteration(); task2.train_iteration()
    assert torch.equal(task.traj.action, task2.traj.action) and torch.equal(task.traj.actor_obs, task2.traj.actor_obs)
    v = task.validate(num_envs=64, seconds=0.2)
    assert np.isfinite(list(v.values())).all()
    npz = str(tmp_path / "actor.npz")
    task.export_actor(npz)
    ex = np.load(npz)
    assert ex["actor.input_proj.weight"].shape == (64, 68) and int(ex["meta.num_inputs"]) == 68


def test_run_mode_view_records_the_policy_rollout(tmp_path):
    """f4, `python -m train run_mode=view` (reference README.md:66-70): launch() with run_mode="view" loads the run directory's checkpoint and
    writes a recording of the deterministic rollout (host/view.py). The recorded positions are the env states the validation rollout went
    through: base height and foot heights from the recording's kinematics equal the kernel's own aux columns, frame by frame; the training
    state is untouched; the recording is reproducible."""
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    from kbot_joystick_amd.spec import layout as L
    run = str(tmp_path / "run_0")
    t = HumanoidWalkingTask.launch(_small(render_length_seconds=1.0), num_iterations=2, run_dir=run, quiet=True)
    p0, it0 = t.params.clone(), t.iteration
    rec = t.view(None, num_envs=4)
    F = rec.qpos.shape[0]
    assert rec.qpos.shape == (51, 4, 27) and rec.xpos.shape == (51, 4, 24, 3) and rec.reward.shape == (50, 4)
    tr = t._valid[3]
    cobs = tr.critic_obs.cpu().numpy()            # row f = what the critic saw at frame f: base position / orientation are the state's own (clean) values
    bp, bq = L.OBS["BASEPOS"][0], L.OBS["BASEQUAT"][0]
    mb = t.model_blob
    for f in (0, 1, 17, 50):
        assert np.array_equal(rec.qpos[f][:, 0:3], cobs[f][:, bp:bp + 3]) and np.array_equal(rec.qpos[f][:, 3:7], cobs[f][:, bq:bq + 4])
        assert np.array_equal(rec.xpos[f][:, int(mb.base_body)].astype(np.float32), cobs[f][:, bp:bp + 3])
    assert np.all(rec.xpos[:, :, int(mb.lfoot_body), 2] > -0.05) and np.all(rec.xpos[:, :, int(mb.base_body), 2] < 1.5)     # a robot on the ground, not a scrambled record
    assert np.array_equal(rec.cmd[3], tr.aux[3][:, L.AUX["CMD"]:L.AUX["CMD"] + 16].cpu().numpy())
    assert torch.equal(t.params, p0) and t.iteration == it0
    rec2 = t.view(None, num_envs=4)
    assert np.array_equal(rec.qpos, rec2.qpos)
    # the launch-level mode: a fresh process-level call that only plays the checkpoint
    v = HumanoidWalkingTask.launch(_small(render_length_seconds=1.0, run_mode="view"), run_dir=run, quiet=True)
    out = os.path.join(run, "view", f"rollout_{it0}")
    assert v.iteration == it0 and os.path.exists(out + ".html") and os.path.exists(out + ".npz")
    z = np.load(out + ".npz")
    assert np.array_equal(z["qpos"], rec.qpos)                                       # same parameters (from ckpt.bin), same seed: same rollout
    with pytest.raises(ValueError, match="run_mode"):
        HumanoidWalkingTask(_small(run_mode="render"))
    # view mode plays the CHECKPOINTED policy: without the run's ckpt.bin it is an error, not a recording of the random initial policy
    with pytest.raises(FileNotFoundError, match="ckpt.bin"):
        HumanoidWalkingTask.launch(_small(render_length_seconds=1.0, run_mode="view"), run_dir=str(tmp_path / "no_such_run"), quiet=True)
    with pytest.raises(FileNotFoundError, match="ckpt.bin"):
        HumanoidWalkingTask.launch(_small(render_length_seconds=1.0, run_mode="view"), run_dir=None, quiet=True)
    assert not os.path.exists(str(tmp_path / "no_such_run" / "view"))
    t.close(); v.close()


def test_launch_loop_with_validation_and_background_checkpoints(tmp_path):
    """launch() as the reference's user runs it (train.py:1783-1790): scalar logging every iteration, a validation rollout every
    valid_every_n_steps iterations, ckpt.bin rewritten every save_every_n_seconds - written by a background thread from a snapshot taken in
    line. The loop's own statistics say what ran; the file on disk at the end is complete and resumes the run bit for bit."""
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    run = str(tmp_path / "run_1")
    t = HumanoidWalkingTask.launch(_small(render_length_seconds=0.4, valid_every_n_steps=3, save_every_n_seconds=1e-4), num_iterations=7, run_dir=run, quiet=True)   # (period far below an iteration of this small task - a few milliseconds since round 6 -: a save is due after every iteration)
    st = t.loop_stats
    assert st["iterations"] == 7 and st["validations"] == 2 and st["checkpoints"] >= 5 and st["env_steps_per_s"] > 0
    assert st["loop_seconds"] >= st["validation_seconds"] + st["checkpoint_seconds"]
    assert getattr(t, "_save_thread", None) is None                    # every writer joined
    ck = os.path.join(run, "checkpoints", "ckpt.bin")
    assert os.path.exists(ck) and not os.path.exists(ck + ".tmp")
    t2 = HumanoidWalkingTask.load_task(ck)
    assert t2.iteration == 7 and torch.equal(t2.params, t.params) and torch.equal(t2.opt_m, t.opt_m)
    t.rollout(); t2.rollout()
    assert torch.equal(t.traj.action, t2.traj.action) and torch.equal(t.traj.aux, t2.traj.aux)
    # a writer that fails is reported by the next wait, not swallowed
    t.save_checkpoint(str(tmp_path / "no_such_dir" / "ckpt.bin"), background=True)
    with pytest.raises((FileNotFoundError, OSError)):
        t.wait_for_checkpoint()
    t.close(); t2.close()


def test_training_iterations_are_not_slower_after_a_validation():
    """The validation / view rollouts run on a second library context (own env rows, workspace, lanes) that stays cached. Round 4's review
    suspected that its idle streams slow every later training iteration (DESIGN.md section 10 had measured such a cliff for extra USER
    streams); measured it does not (tools/validate_cliff.py -> profiles/r05a_validate_cliff.json: +0.2 % / +0.0 % / -0.1 %; the driver's own
    bench line carries `train_loop.vs_headline`, launch() with validations and checkpoints against the bare loop). This test keeps the
    FUNCTIONAL parts - the cached context, close_validation(), re-creation on demand - and a coarse guard against a real cliff: a wall-clock
    bound of 10 %, five times the box-to-box spread, so it cannot go red for no code reason (the 2 % bound of round 5 could)."""
    import time
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config
    task = HumanoidWalkingTask(launch_config(num_envs=8192, robot="kbot-headless", fixed_command=(0.5, 0.0, 0.0)))

    def leg(k=3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(k):
            task.train_iteration()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k
    for _ in range(2):
        task.train_iteration()
    before = min(leg(), leg())
    task.validate()
    assert getattr(task, "_valid", None) is not None
    after_validate = min(leg(), leg())
    task.view()
    after_view = leg()
    task.close_validation()
    assert getattr(task, "_valid", None) is None
    task.validate(num_envs=16, seconds=0.2)          # built again on demand
    task.close()
    assert after_validate <= 1.10 * before and after_view <= 1.10 * before, (before, after_validate, after_view)


def test_default_schedule_survives_kernel_serialisation():
    """The default schedule under HIP's own serialisation (AMD_SERIALIZE_KERNEL=3: the host waits for every kernel before it enqueues the
    next - a common debugging setting) in a child process: the persistent recurrences, whose workgroups wait for each other INSIDE one
    launch, and the multi-lane update must run to the same kind of result. (This is host-order serialisation. `rocprofv3 --pmc` serialises at
    the queues, in readiness order: there a kernel that waits for ANOTHER LAUNCH could be dispatched first and spin to its bound. The schedule
    contains no such kernel - the gate kernels of rounds 3 / 4 are gone, DESIGN.md section 2 states the invariant - and `tools/profile_all.sh`
    runs the counter passes through it.)"""
    import subprocess, sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import torch\n"
            "from kbot_joystick_amd.host.task import HumanoidWalkingTask, launch_config\n"
            "t = HumanoidWalkingTask(launch_config(num_envs=128, batch_size=64, hidden_size=256, rollout_length_seconds=0.2, robot='kbot-headless', seed=3, num_passes=1))\n"
            "t.train_iteration(); t.train_iteration(); torch.cuda.synchronize()\n"
            "assert torch.isfinite(t.params).all() and torch.isfinite(t.metrics).all()\n"
            "print('SERIAL_OK', float(t.metrics[0]))\n") % ROOT
    env = {k: v for k, v in os.environ.items() if not k.startswith("KBJ_") or k == "KBJ_LIB_NAME"}
    env.update(AMD_SERIALIZE_KERNEL="3", AMD_SERIALIZE_COPY="3")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "SERIAL_OK" in out.stdout, (out.stdout[-300:], out.stderr[-600:])


@pytest.mark.parametrize("size", ["256 envs x 50 steps, full kbot on the terrain", "configs[1]: 8192 envs x 100 steps"])
def test_reference_reward_classes_on_the_trajectory_reproduce_the_kernel(size):
    """f3: with `record_state` the Python reward terms see a ksim-shaped Trajectory (host/trajectory.py). Two real rollouts of the full kbot on
    the sine terrain (sampler commands, pushes, terminations - the initial policy falls): (a) the recorded qpos / qvel are the env rows after
    the step; (b) the forward kinematics over the recorded positions reproduce the poses the kernel itself wrote into the aux record;
    (c) the reference's twelve reward classes, restated in torch with the reference's attribute names (train.py:138-506), reproduce
    rewards_kernel term by term to 2e-4, carries of the stateful ones included; (d) a user term sees the same object."""
    import torch
    from kbot_joystick_amd.host import trajectory as TJ
    from examples import reference_rewards as RR          # the reference's reward classes: example material, not product code
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    from kbot_joystick_amd.spec import constants, layout as L
    seen = {}

    class Probe:                      # a user term in ksim's Reward protocol, written against the reference's field names
        scale = 0.0

        def get_reward(self, trajectory):
            seen["type"] = type(trajectory).__name__
            seen["qpos"] = tuple(trajectory.qpos.shape)
            return -trajectory.qvel[..., 6:].square().sum(dim=-1) * 0 + trajectory.xpos[..., 1, 2] * 0
    big = size.startswith("configs[1]")
    if big:      # the BASELINE workload: kbot-headless, flat ground, fixed command (0.5, 0, 0), 8192 envs x 100 steps
        from kbot_joystick_amd.host.task import launch_config
        cfg = launch_config(num_envs=8192, robot="kbot-headless", fixed_command=(0.5, 0.0, 0.0), record_state=True, log_reward_components=True, seed=11)
    else:
        cfg = _small(num_envs=256, batch_size=64, rollout_length_seconds=1.0, robot="kbot", terrain="sine", record_state=True, log_reward_components=True, seed=11)
    NE = cfg.num_envs
    task = HumanoidWalkingTask(cfg, extra_rewards={"probe": Probe()})
    terms = RR.reference_rewards(task.model_blob, ctrl_dt=cfg.ctrl_dt)
    A, Q, T = L.AUX, L.QSTATE, task.T
    carries, ndone = {}, 0
    for rollout in range(2):
        task.rollout()
        task.ctx.synchronize()
        tr = task.trajectory()
        assert isinstance(tr, TJ.Trajectory) and seen == {"type": "Trajectory", "qpos": (T, NE, 27)}
        aux = task.traj.aux[:T]
        # (a) the last step's record = the env rows (envs that were not reset by that step)
        _, es = task.ctx.env_get_state()
        alive = (aux[T - 1, :, A["DONE"]] == 0).cpu().numpy()
        assert alive.sum() > 100
        assert np.array_equal(tr.qpos[T - 1].cpu().numpy()[alive], es[alive, L.ES["QPOS"]:L.ES["QPOS"] + 27])
        assert np.array_equal(tr.qvel[T - 1].cpu().numpy()[alive], es[alive, L.ES["QVEL"]:L.ES["QVEL"] + 26])
        assert torch.equal(tr.qvel[..., :6], aux[..., A["QVEL"]:A["QVEL"] + 6]) and torch.equal(tr.qpos[..., 17:27], aux[..., A["ARMQ"]:A["ARMQ"] + 10])
        # (b) kinematics of the step's last forward pass
        mb = task.model_blob
        for body, zc, qc in ((int(mb.base_body), "BASEZ", "BQUAT"), (int(mb.lfoot_body), "LFZ", "LFQUAT"), (int(mb.rfoot_body), "RFZ", "RFQUAT")):
            assert float((tr.xpos[..., body, 2] - aux[..., A[zc]]).abs().max()) < 2e-6
            qk = aux[..., A[qc]:A[qc] + 4]
            sgn = torch.sign((tr.xquat[..., body, :] * qk).sum(-1, keepdim=True))
            assert float((tr.xquat[..., body, :] - sgn * qk).abs().max()) < 2e-6
        # (c) the twelve terms
        total = torch.zeros_like(task.traj.reward)
        for k, (name, term) in enumerate(terms.items()):
            if hasattr(term, "get_reward_stateful"):
                if name not in carries:
                    carries[name] = term.initial_carry(NE, task.device)
                r, carries[name] = term.get_reward_stateful(tr, carries[name])
            else:
                r = term.get_reward(tr)
            err = float((r - task.traj.comps[..., k]).abs().max())
            assert err < 2e-4, (rollout, name, constants.REWARD_NAMES[k], err)
            total += term.scale * r
        assert float((total - task.traj.reward).abs().max()) < 2e-4
        ndone += int(tr.done.sum())
        task.iteration += 1
    assert ndone > 20                                              # terminations (and the carries' done handling) were exercised
    if big:
        task.close()
        return
    # the step-by-step path (user terms) records the same states as the fused rollout
    t1 = HumanoidWalkingTask(_small(num_envs=64, record_state=True, seed=5))
    t2 = HumanoidWalkingTask(_small(num_envs=64, record_state=True, seed=5), extra_terminations={"never": lambda state, level: torch.zeros(state.N, device=state.done.device)})
    t1.rollout(); t2.rollout()
    assert torch.equal(t1.traj.qstate, t2.traj.qstate) and float(t1.traj.qstate.abs().sum()) > 0
    # without the record the narrower view is what terms get, and asking for the ksim-shaped one says why it is not there
    t3 = HumanoidWalkingTask(_small(num_envs=64, seed=5))
    t3.rollout()
    assert type(t3.trajectory()).__name__ == "TrajectoryView"
    with pytest.raises(ValueError, match="record_state"):
        TJ.Trajectory(t3.traj, t3.T, t3.model_blob)
    # get_rewards() entries are executable: an EDITED reward table (reward_scales / reward_params) built into torch terms reproduces the kernel that
    # runs the same table; and a user replaces a built-in term by zeroing its scale and passing the built (then edited) term as an extra reward
    edits = dict(reward_scales={"feet_airtime": 2.0, "torque": 0.0}, reward_params={"base_height": {"standard_height": 0.85, "error_scale": 0.05},
                                                                                     "single_contact": {"grace_period": 0.5}, "linvel": {"error_scale": 0.3}})
    t4 = HumanoidWalkingTask(_small(num_envs=128, rollout_length_seconds=1.0, record_state=True, log_reward_components=True, seed=9, **edits))
    built = {k: spec.build(t4.model_blob) for k, spec in t4.get_rewards().items()}
    assert built["feet_airtime"].scale == 2.0 and built["base_height"].standard_height == pytest.approx(0.85) and built["single_contact"].grace_period == pytest.approx(0.5)
    t4.rollout(); t4.ctx.synchronize()
    tr4, total, carries4 = t4.trajectory(), torch.zeros_like(t4.traj.reward), {}
    for k, (name, term) in enumerate(built.items()):
        r = term.get_reward_stateful(tr4, term.initial_carry(128, t4.device))[0] if hasattr(term, "get_reward_stateful") else term.get_reward(tr4)
        assert float((r - t4.traj.comps[..., k]).abs().max()) < 2e-4, name
        total += term.scale * r
    assert float((total - t4.traj.reward).abs().max()) < 2e-4
    swapped = dict(edits, reward_scales=dict(edits["reward_scales"], base_height=0.0))
    t5 = HumanoidWalkingTask(_small(num_envs=128, rollout_length_seconds=1.0, record_state=True, seed=9, **swapped), extra_rewards={"base_height": built["base_height"]})
    t5.rollout(); t5.ctx.synchronize()
    assert float((t5.traj.reward - t4.traj.reward).abs().max()) < 2e-4       # the torch term in place of the kernel's: the same reward
    for t in (task, t1, t2, t3, t4, t5):
        t.close()


def test_python_reset_terms():
    """f3: user-written Reset terms in the reference's protocol (train.py:833-844 `Reset.__call__(data, curriculum_level, rng) -> data`) on top of the
    built-in resets, through kbj_env_get_qstate / kbj_env_set_qstate. (a) A term that returns its data unchanged leaves the run identical to the stock
    one (state rows, aux record and actions bit for bit; derived critic entries to 1e-6: the forward pass behind the reset is compiled into two
    kernels). (b) The reference's own PlaneXYPositionReset body, restated per env (`qpos_j.at[0:1].set(new_x)`), moves exactly the envs whose episode
    starts - their state rows and the base position the critic sees - and nobody else. (c) A term that also sets velocities shows up in qvel."""
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    from kbot_joystick_amd.host.traj_view import ResetData, per_env_reset, update_data_field
    from kbot_joystick_amd.spec import layout as L
    kw = dict(num_envs=256, batch_size=64, rollout_length_seconds=1.0, seed=6)
    stock = HumanoidWalkingTask(_small(**kw))
    ident = HumanoidWalkingTask(_small(**kw), extra_resets=[lambda data, level, rng: data])
    for it in range(2):
        stock.rollout(); ident.rollout()
        torch.cuda.synchronize()
        for name in ("aux", "actor_obs", "action", "logp", "reward"):
            assert torch.equal(getattr(stock.traj, name), getattr(ident.traj, name)), (it, name)
        assert float((stock.traj.critic_obs - ident.traj.critic_obs).abs().max()) < 1e-6
        stock.iteration += 1; ident.iteration += 1
    es, ei = stock.ctx.env_get_state()[1], ident.ctx.env_get_state()[1]
    assert np.array_equal(es.view(np.uint32), ei.view(np.uint32))
    assert int((stock.traj.done != 0).sum()) > 20

    class PlaneXYPositionReset:            # train.py:827-844, per env; the two uniform draws come in as extras (torch.vmap has no per-example generator)
        def __init__(self, x_range, y_range):
            self.x_range, self.y_range = x_range, y_range

        def _one(self, data, curriculum_level, rng, new_x, new_y):
            qpos_j = data.qpos
            qpos_j = torch.cat([new_x, new_y, qpos_j[2:]])          # qpos_j.at[0:1].set(new_x); qpos_j.at[1:2].set(new_y)
            return update_data_field(data, "qpos", qpos_j)

        def __call__(self, data, curriculum_level, rng):
            n = data.qpos.shape[0]
            new_x = (torch.rand(n, 1, generator=rng, device=data.qpos.device) * 2 - 1) * self.x_range
            new_y = (torch.rand(n, 1, generator=rng, device=data.qpos.device) * 2 - 1) * self.y_range
            return per_env_reset(self._one)(data, curriculum_level, rng, extras=(new_x, new_y))

    def spin(data, level, rng):            # (c) a second term in the list: fresh episodes start with a yaw rate
        v = data.qvel.clone(); v[:, 5] = 0.75
        return ResetData(data.qpos, v)
    user = HumanoidWalkingTask(_small(**kw), extra_resets=[PlaneXYPositionReset(3.0, 0.5), spin])
    bp = L.OBS["BASEPOS"][0]
    seen = 0
    for it in range(2):
        user.rollout(); torch.cuda.synchronize()
        T = user.T
        done = user.traj.aux[:T, :, L.AUX["DONE"]] != 0
        nxt = user.traj.critic_obs[1:T + 1, :, bp:bp + 2]           # base xy of the row after each step
        assert bool((nxt[done][:, 0].abs() <= 3.0).all()) and bool((nxt[done][:, 1].abs() <= 0.5).all())
        assert float(nxt[done][:, 0].abs().max()) > 0.5             # far outside the built-in reset's +-0.1 m: the term's draw, not the kernel's
        av = L.OBS["ANGVEL"][0]
        assert bool((user.traj.critic_obs[1:T + 1, :, av + 2][done] == 0.75).all())      # the critic sees the yaw rate of the fresh state
        if it == 0:                                                 # row 0 of the first rollout: every env starts an episode
            assert float(user.traj.critic_obs[0, :, bp].abs().max()) > 0.5 and bool((user.traj.critic_obs[0, :, av + 2] == 0.75).all())
        seen += int(done.sum())
        user.iteration += 1
    assert seen > 20
    # envs that did not finish keep their own trajectory: a running env's position changes by a step's worth, never by metres
    run = ~done[:-1] & ~done[1:]
    step_xy = (user.traj.critic_obs[2:T + 1, :, bp:bp + 2] - user.traj.critic_obs[1:T, :, bp:bp + 2]).norm(dim=-1)
    assert float(step_xy[run].max()) < 0.2
    _, es_u = user.ctx.env_get_state()
    qp = torch.empty(256, 27, device="cuda"); qv = torch.empty(256, 26, device="cuda")
    user.ctx.env_get_qstate(qp, qv); torch.cuda.synchronize()
    assert np.array_equal(qp.cpu().numpy(), es_u[:, L.ES["QPOS"]:L.ES["QPOS"] + 27]) and np.array_equal(qv.cpu().numpy(), es_u[:, L.ES["QVEL"]:L.ES["QVEL"] + 26])
    user.train_iteration(); torch.cuda.synchronize()                # a full iteration (and a validation rollout) with the terms in place
    assert torch.isfinite(user.params).all() and np.isfinite(list(user.validate(num_envs=64, seconds=0.4).values())).all()
    with pytest.raises(KeyError):
        update_data_field(ResetData(qp, qv), "ctrl", qp)
    for t in (stock, ident, user):
        t.close()


def _recording_terms(log, into=None):
    """One neutral user term of each kind as HumanoidWalkingTask keywords; every call appends (kind, the seed of the generator it got, or None)."""
    import torch

    def termination(state, curriculum_level):
        log.append(("termination", None))
        return torch.zeros(state.N, device="cuda")

    def reset(data, curriculum_level, rng):
        log.append(("reset", rng.initial_seed()))
        return data

    class Command:
        def initial_command(self, state, curriculum_level, rng):
            log.append(("initial_command", rng.initial_seed()))
            return torch.zeros(state.N, L.NCMD, device="cuda")

        def __call__(self, prev_command, state, curriculum_level, rng):
            log.append(("command", rng.initial_seed()))
            return prev_command

    class Observation:
        def observe(self, state, curriculum_level, rng):
            log.append(("observation", None if rng is None else rng.initial_seed()))
            return torch.zeros(state.N, 1, device="cuda")

    return dict(extra_terminations={"never": termination}, extra_resets=[reset], command=Command(),
                extra_observations={"zero": (Observation(), into)})


_SEED, _T = 4, 3          # _small()'s seed (rank 0), and T of rollout_length_seconds = 0.06


def _command_seed(step_index):
    return (_SEED * 2654435761 + step_index * 40503 + 0) & 0x7FFFFFFFFFFFFFFF


def _reset_seed(step_index):
    return (_SEED * 2246822519 + step_index * 3266489917 + 0) & 0x7FFFFFFFFFFFFFFF


def test_user_term_order_and_generator_seeds_in_training():
    """The step-wise rollout calls the user terms as terminations -> resets -> command -> observations after every control step, resets ->
    command -> observations on row 0 of the FIRST rollout only, and seeds the generators of step `iteration * T + row` as written above."""
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    log = []
    task = HumanoidWalkingTask(_small(rollout_length_seconds=0.06), **_recording_terms(log))
    assert task.T == _T and log == []
    task.rollout(); task.iteration += 1; task.rollout()
    task.ctx.synchronize()

    def step(k):
        return [("termination", None), ("reset", _reset_seed(k)), ("initial_command", _command_seed(k)), ("command", _command_seed(k)), ("observation", None)]
    expect = [("reset", _reset_seed(0)), ("initial_command", _command_seed(0)), ("observation", None)]
    for iteration in range(2):                      # the second rollout has no prologue calls
        for row in range(1, _T + 1):
            expect += step(iteration * _T + row)
    assert log == expect
    task.close()


def test_user_term_order_and_generator_seeds_in_validation():
    """validate() calls the user terms as resets -> observations -> command (NOT training's order), the same on row 0 of every call, never
    the termination terms, and an observation term only when it feeds the networks; generators are seeded for step `seed_offset + row`."""
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    log, off = [], 7919
    task = HumanoidWalkingTask(_small(rollout_length_seconds=0.06, extra_actor_obs=1, extra_critic_obs=1), **_recording_terms(log, "both"))
    for _ in range(2):                              # the row-0 prologue runs on every call
        del log[:]
        task.validate(num_envs=32, seconds=0.06)
        expect = [("reset", _reset_seed(off)), ("initial_command", _command_seed(off)), ("observation", None)]
        for row in range(1, _T + 1):
            k = off + row
            expect += [("reset", _reset_seed(k)), ("observation", None), ("initial_command", _command_seed(k)), ("command", _command_seed(k))]
        assert log == expect
    task.close()
    unrouted = HumanoidWalkingTask(_small(rollout_length_seconds=0.06), **_recording_terms(log))
    del log[:]
    unrouted.validate(num_envs=32, seconds=0.06)
    kinds = [kind for kind, _ in log]
    assert kinds == ["reset", "initial_command"] + ["reset", "initial_command", "command"] * _T
    unrouted.close()


def test_stepwise_rollout_with_a_silent_term_equals_the_fused_one():
    """A task whose only user term is a termination that never fires runs the step-wise loop; its trajectory and env rows are the fused
    kbj_rollout's bit for bit, and the step-wise validation returns what the fused one returns."""
    import torch
    from kbot_joystick_amd.host.task import HumanoidWalkingTask
    stock = HumanoidWalkingTask(_small(rollout_length_seconds=0.06))
    user = HumanoidWalkingTask(_small(rollout_length_seconds=0.06), extra_terminations={"never": lambda state, level: torch.zeros(state.N, device="cuda")})
    for it in range(2):
        stock.rollout(); user.rollout()
        torch.cuda.synchronize()
        for name in ("aux", "actor_obs", "critic_obs", "action", "logp", "value", "reward"):
            assert torch.equal(getattr(stock.traj, name), getattr(user.traj, name)), (it, name)
        stock.iteration += 1; user.iteration += 1
    es, eu = stock.ctx.env_get_state()[1], user.ctx.env_get_state()[1]
    assert np.array_equal(es.view(np.uint32), eu.view(np.uint32))
    assert user.validate(num_envs=32, seconds=0.2, _stepwise=True) == user.validate(num_envs=32, seconds=0.2)
    stock.close(); user.close()


def test_example_with_all_six_user_term_protocols_runs():
    """examples/custom_terms.py: a reward (per env on the ksim-shaped Trajectory), a termination (per env on physics_data names), a reset, an observation routed
    into the critic, and a command term, all written in the reference's protocols, train together."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "custom_terms.py"), "2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "custom terms ok" in out.stdout, (out.stdout[-1500:], out.stderr[-2500:])
    assert "iter 2:" in out.stdout
