"""The deployed actor in numpy float64: `init_fn` / `step_fn` restated from convert.py:74-119 with Actor.forward (train.py:913-941) and
the observation normalisers (train.py:1329-1349). Test infrastructure: tests/test_deploy_host.py pins it against the torch oracle
(oracle/nn.py, an independent restatement), tests/test_gpu_deploy.py holds kbj_deploy_step to it.

Flat carry of one row = ravel_pytree(Carry(actor_carry [depth][2][H], lpf [20])): per layer h then c, then the low-pass floats."""
import numpy as np

from kbot_joystick_amd.spec import layout as L

NU = 20


def actor_leaves(params, H, depth):
    """name -> float64 array of the actor's leaves, sliced from a flat parameter vector (the actor's prefix is enough)."""
    out, off = {}, 0
    for name, shape in L.param_leaves(H, depth):
        if not name.startswith("actor."):
            break
        n = int(np.prod(shape))
        out[name] = np.asarray(params[off:off + n], np.float64).reshape(shape)
        off += n
    return out


def carry_size(H, depth):
    return depth * 2 * H + NU                                                            # convert.py:71


def init(n, H, depth):
    return np.zeros((n, carry_size(H, depth)))                                           # convert.py:74-82


def joint_norm(model):
    bias, lo, hi = (np.array(list(v), np.float64) for v in (model.joint_bias, model.joint_lo, model.joint_hi))
    return bias, np.maximum(bias - lo, hi - bias)                                        # train.py:1330-1332


def pack(model, joint_angles, joint_angular_velocities, projected_gravity, gyroscope, command):
    """convert.py:93-105: the 65-float observation rows [n, 65] from the raw inputs."""
    ja, jv, pg, gy, cmd = (np.asarray(v, np.float64) for v in (joint_angles, joint_angular_velocities, projected_gravity, gyroscope, command))
    bias, rng = joint_norm(model)
    cmd_zero = (np.sqrt((cmd[:, :3] ** 2).sum(-1)) < 1e-3).astype(np.float64)[:, None]    # convert.py:93
    roll = np.arctan2(pg[:, 1], -pg[:, 2])                                                # train.py:1339-1341
    pitch = np.arctan2(-pg[:, 0], np.sqrt(pg[:, 1] ** 2 + pg[:, 2] ** 2))
    unit = pg / np.sqrt((pg ** 2).sum(-1, keepdims=True))
    return np.concatenate([(ja - bias) / rng, jv / 10.0, roll[:, None], pitch[:, None], unit, gy, cmd_zero, cmd], axis=-1)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward(p, model, alpha, H, depth, obs, carry):
    """Actor.forward on packed rows (train.py:913-941) with the flat carry; returns (mode, new flat carry)."""
    hc, lpf = carry[:, :2 * depth * H].reshape(-1, depth, 2, H), carry[:, 2 * depth * H:]
    x = obs @ p["actor.input_proj.weight"].T + p["actor.input_proj.bias"]                 # train.py:916
    new = []
    for l in range(depth):                                                                # train.py:918-921, equinox LSTMCell: i, f, g, o
        g = x @ p[f"actor.rnns.{l}.weight_ih"].T + hc[:, l, 0] @ p[f"actor.rnns.{l}.weight_hh"].T + p[f"actor.rnns.{l}.bias"]
        i, f, gg, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:])
        c = f * hc[:, l, 1] + i * gg
        h = o * np.tanh(c)
        new += [h, c]
        x = h
    out = x @ p["actor.output_proj.weight"].T + p["actor.output_proj.bias"]               # train.py:922
    mean = out[:, :NU] + joint_norm(model)[0]                                             # train.py:925, 932-933
    mean[:, 10:] += obs[:, -10:]
    y = lpf + alpha * (mean - lpf)                                                        # ksim.lowpass_one_pole, train.py:936
    return y, np.concatenate(new + [y], axis=-1)                                          # dist.mode(), the new flat carry (convert.py:116-119)


def step(params, model, alpha, H, depth, joint_angles, joint_angular_velocities, projected_gravity, gyroscope, command, carry):
    """step_fn (convert.py:84-119): (action [n, 20], new flat carry [n, carry_size]) in float64."""
    p = params if isinstance(params, dict) else actor_leaves(params, H, depth)
    obs = pack(model, joint_angles, joint_angular_velocities, projected_gravity, gyroscope, command)
    return forward(p, model, float(alpha), H, depth, obs, np.asarray(carry, np.float64))


def random_sensors(model, rng, n, scale=1.0):
    """Seeded sensor rows in their physical ranges (float32): joint angles inside the limits around the bias, joint velocities of a few
    rad/s, gravity (9.81 m/s^2) tilted up to ~0.5 rad, body rates ~1 rad/s, a joystick command with non-zero arm targets."""
    bias, lo, hi = (np.array(list(v), np.float64) for v in (model.joint_bias, model.joint_lo, model.joint_hi))
    ja = np.clip(bias + rng.uniform(-0.5, 0.5, (n, NU)) * scale, lo, hi)
    jv = rng.normal(size=(n, NU)) * 2.0 * scale
    tilt, az = rng.uniform(0.0, 0.5, n) * scale, rng.uniform(-np.pi, np.pi, n)
    pg = 9.81 * np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), -np.cos(tilt)], -1)
    gy = rng.normal(size=(n, 3)) * scale
    cmd = np.concatenate([rng.uniform(-0.5, 1.2, (n, 1)), rng.uniform(-0.5, 0.5, (n, 1)), rng.uniform(-1, 1, (n, 1)), rng.uniform(-0.25, 0.05, (n, 1)),
                          rng.uniform(-0.25, 0.25, (n, 2)), rng.uniform(0.05, 0.6, (n, 10)) * rng.choice([-1.0, 1.0], (n, 10))], -1)
    return tuple(np.ascontiguousarray(v, np.float32) for v in (ja, jv, pg, gy, cmd))
