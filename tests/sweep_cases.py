"""The batch of a command sweep, shared by the tests that solve one (tests/test_gpu_command_sweep.py, test_gpu_sweep_select.py,
test_gpu_stream_order.py and others)."""
import numpy as np

from hector_simulation_amd import synthetic


def sweep_fields(groups: int, k: int, h: int, gait: str, seed: int, scale: float = 1.0) -> dict:
    """`groups` random states (synthetic.make_batch), each under `k` velocity / yaw-rate commands: every field repeated k times,
    the reference trajectory rebuilt per command exactly as make_batch builds it."""
    base = synthetic.make_batch(groups, h, gait, seed=seed, phase="random")
    f = {key: np.repeat(np.asarray(v), k, axis=0) for key, v in base.items()}
    rng = np.random.default_rng(seed + 99)
    b = groups * k
    vx = rng.uniform(-0.5 * scale, 0.5 * scale, b)
    vy = rng.uniform(-0.2 * scale, 0.2 * scale, b)
    yr = rng.uniform(-0.3 * scale, 0.3 * scale, b)
    tr = f["traj"].reshape(b, h, 12).copy()
    p = f["p"]
    steps = np.arange(h)[None, :]
    tr[:, :, 9], tr[:, :, 10], tr[:, :, 8] = vx[:, None], vy[:, None], yr[:, None]
    tr[:, :, 3] = p[:, 0:1] + steps * synthetic.DT_MPC * vx[:, None]
    tr[:, :, 4] = p[:, 1:2] + steps * synthetic.DT_MPC * vy[:, None]
    tr[:, 1:, 2] = tr[:, 0:1, 2] + steps[:, 1:] * synthetic.DT_MPC * yr[:, None]
    f["traj"] = tr.reshape(b, 12 * h)
    return f
