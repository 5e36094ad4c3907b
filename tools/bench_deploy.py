"""Latency of the deployed actor step, kbj_deploy_step (one launch, csrc/kbj_deploy.h), beside kbj_policy_step(argmax=1) at the same N from the
same process. kbj_policy_step is the training path and the only other way to step a policy: it ALSO runs the critic and needs a context
whose num_envs is N, so the two columns are what a user pays either way, not the same work.
Two figures per path and N, both on a real device only:
  call : median of a host clock around ONE call that ends in a device synchronise (joystick in the loop: the next sensors wait for the action)
  b2b  : HIP events around the same number of calls issued back to back, per call (launch cost hidden, the device's own time)
usage: bench_deploy.py [H] [depth] [calls]     (N = 1, 8, 64; prints one JSON line per N)"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from kbot_joystick_amd.spec import compiler, layout as L
from kbot_joystick_amd.host import binding as B, buffers

H = int(sys.argv[1]) if len(sys.argv) > 1 else 256
D = int(sys.argv[2]) if len(sys.argv) > 2 else 2
K = max(200, int(sys.argv[3])) if len(sys.argv) > 3 else 300
if not torch.cuda.is_available():
    sys.exit("bench_deploy.py measures on a HIP device; there is none")
dev = "cuda:0"
m = compiler.load_model("kbot-headless")


def measure(fn, sync):
    for _ in range(50):
        fn()
    sync()
    calls = []
    for _ in range(K):
        t0 = time.perf_counter()
        fn(); sync()
        calls.append((time.perf_counter() - t0) * 1e6)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(K):
        fn()
    e1.record(); sync()
    q = statistics.quantiles(calls, n=10)
    return dict(call_us_median=round(statistics.median(calls), 2), call_us_p10=round(q[0], 2), call_us_p90=round(q[-1], 2), b2b_us=round(e0.elapsed_time(e1) / K * 1e3, 2))


for N in (1, 8, 64):
    cfg = L.default_config(num_envs=N, batch_size=N, hidden_size=H, depth=D)
    ctx = B.Context(m, cfg, 0, torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=dev).manual_seed(0)
    params = torch.zeros(ctx.param_count(), device=dev); ctx.init_params(1, params)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    ja, jv, gy, cmd = r(N, 20) * 0.3, r(N, 20), r(N, 3), r(N, 16) * 0.3
    pg = torch.tensor([[0.5, -0.3, -9.7]], device=dev).repeat(N, 1)
    flat, act = torch.zeros(N, ctx.deploy_carry_size(), device=dev), torch.zeros(N, 20, device=dev)
    ctx.deploy_init(N, flat)
    a, c = torch.zeros(N, L.LD_ACTOR, device=dev), torch.zeros(N, L.LD_CRITIC, device=dev)
    a[:, :65] = r(N, 65); c[:, :475] = r(N, 475)
    carry = buffers.CarryBuffers(N, H, D, dev)
    act2, lp, v = torch.zeros(N, 20, device=dev), torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    deploy = lambda: ctx.deploy_step(params, ja, jv, pg, gy, cmd, N, flat, flat, act)
    policy = lambda: ctx.policy_step(params, a, c, carry.c, 1, 0, True, act2, lp, v)
    res = {}
    for rep in range(2):                       # alternate the two paths; keep the second round (both warm, same machine state)
        res["kbj_deploy_step"] = measure(deploy, ctx.synchronize)
        res["kbj_policy_step_argmax"] = measure(policy, ctx.synchronize)
    print(json.dumps(dict(H=H, depth=D, N=N, calls=K, **res, checksum=[round(float(act.sum()), 5), round(float(act2.sum()), 5)])))
    ctx.close()
