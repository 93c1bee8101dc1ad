"""The batched prologue of the assembly's scalar front (csrc/hmpc_front.hip, ahead of the fast two-contact solve kernels) on the GPU.
All comparisons are bitwise.
 (a) its blocks (hmpc_debug_front_scalars), turned back into x0 / Acd / Bcd / Fc the way the solve kernel's scatter does, against the
     oracle's arrays, and its prefix counts against a plain count of the gait bytes;
 (b) solves with the prologue on (the default) against off (hmpc_debug_set_front_prologue: every kernel runs the two stages itself), on
     fresh handles: forces, status words, the binary64 solution and objective, and -- through a second solve that starts from it -- the
     tick-to-tick working set;
 (c) handle state: a second batch on another, busy stream equals a fresh handle's."""
import numpy as np
import pytest

import front_cases as fc
import irregular_gaits as ig
import stream_cases as sc
from hector_simulation_amd import interface, records, synthetic

pytestmark = pytest.mark.gpu
DT, FMAX = synthetic.DT_MPC, synthetic.F_MAX
IPW = 16  # instances per workgroup of front_scalars_kernel (csrc/hmpc_front.h FRONT_IPW)


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("gait,h", [("standing", 10), ("walking", 10), ("walking", 20)])
def test_blocks_against_the_oracle(oracle, gait, h):
    nb = 48
    rec = records.pack_records(synthetic.make_batch(nb, h, gait, seed=370 + h, phase="random"), h)
    mpc = interface.BatchedMPC(DT, h, FMAX, nb)
    mpc.upload(rec)
    blk = mpc.debug_front_scalars()
    mpc.close()
    got = fc.arrays_from_blocks(blk, rec, DT, fc.oracle_params(oracle))
    want = fc.expected(oracle, rec, h)
    for k in want:
        np.testing.assert_array_equal(bits(got[k]), bits(want[k]), err_msg=k)
    gaitb = rec[:, 4 * (54 + 12 * h):4 * (54 + 12 * h) + 2 * h].reshape(nb, h, 2) != 0  # (f_max 500: a leg-step is in stance iff its byte is set)
    nst = gaitb.sum(axis=2)
    before = np.cumsum(nst, axis=1) - nst
    np.testing.assert_array_equal(blk["pre_nl"][:, :h], before)
    np.testing.assert_array_equal(blk["pre_nv"][:, :h], 6 * before)
    np.testing.assert_array_equal(blk["pre_st"][:, :h], gaitb[..., 0] + 2 * gaitb[..., 1])
    assert not blk["pre_nl"][:, h:].any() and not blk["pre_nv"][:, h:].any() and not blk["pre_st"][:, h:].any()
    np.testing.assert_array_equal(blk["nls"], nst.sum(axis=1))
    np.testing.assert_array_equal(blk["n"], 6 * nst.sum(axis=1))


# ------------------------------------------------------------------------------------------------ (b)
def solve_twice(rec, h, prologue, setup=None, device=False, hint=None):
    """A fresh handle with the prologue on or off: two solves with the tick-to-tick working set carried, everything downloaded."""
    nb = rec.shape[0]
    mpc = interface.BatchedMPC(DT, h, FMAX, nb)
    keep = []
    try:
        mpc.debug_set_front_prologue(prologue)
        interface._check(mpc.L.hmpc_enable_f64_output(mpc.h), "hmpc_enable_f64_output")
        mpc.set_tick_warm_start(True)
        if setup:
            keep.append(setup(mpc))
        if device:
            d_rec = sc.torch_().from_numpy(np.ascontiguousarray(rec)).cuda()
            mpc.set_device_records(d_rec.data_ptr(), nb, max_reduced_vars=-1 if hint is None else hint, keepalive=d_rec)
        else:
            mpc.upload(rec)
            if hint is not None:
                interface._check(mpc.L.hmpc_set_max_reduced_vars(mpc.h, hint), "hint")
        out = {}
        for tick in (1, 2):
            mpc.solve()
            out[f"forces{tick}"], out[f"status{tick}"] = mpc.download()
            out[f"x64_{tick}"], out[f"obj64_{tick}"] = mpc.download_f64()
        return out
    finally:
        mpc.close()


def assert_on_equals_off(rec, h, **kw):
    on, off = solve_twice(rec, h, True, **kw), solve_twice(rec, h, False, **kw)
    sc.assert_same(on, off, "prologue on against off")
    assert np.abs(on["forces1"]).max() > 1.0  # (something was solved)
    return on


def standing(nb, h=10, seed=380):
    return records.pack_records(synthetic.make_batch(nb, h, "standing", seed=seed, yaw_rate_cmd=True), h)


@pytest.mark.parametrize("nb", [1, IPW - 1, IPW, IPW + 1, 33])
def test_standing_batches_around_the_prologues_workgroup(nb):
    assert_on_equals_off(standing(nb), 10)  # (variant 1)


def test_walking_on_the_small_variant():
    rec = records.pack_records(synthetic.make_batch(40, 10, "walking", seed=381, phase="random"), 10)
    assert_on_equals_off(rec, 10, hint=60)  # (variant 0)


@pytest.mark.parametrize("hint", [60, 120])
def test_single_support_over_twenty_steps(hint):
    """Variant 3: one leg in stance over all twenty steps (120 variables).  Variant 2 holds ten leg-steps: single support over half the
    horizon and less -- 4 .. 10 stance leg-steps at random places of the twenty steps."""
    if hint == 120:
        rec = records.pack_records(synthetic.make_batch(24, 20, "single", seed=382, phase="random"), 20)
    else:
        rng = np.random.default_rng(382)
        rec = ig.pack(ig.fields(20, 2, [ig.exact_count(20, 2, 4 + i % 7, rng) for i in range(24)], 382), 20, 2)
    assert_on_equals_off(rec, 20, hint=hint)


@pytest.mark.parametrize("h", [10, 20])
def test_device_records_without_a_hint_run_the_size_classes(h):
    """Standing and walking mixed (h = 20: single and double support, so that the wide variant runs its in-kernel path inside the same solve)."""
    a = synthetic.make_batch(20, h, "standing", seed=383, yaw_rate_cmd=True)
    b = synthetic.make_batch(20, h, "walking" if h == 10 else "single", seed=384, phase="random")
    f = {k: np.concatenate([np.asarray(a[k]), np.asarray(b[k])])[np.random.default_rng(385).permutation(40)] for k in a}
    assert_on_equals_off(records.pack_records(f, h), h, device=True)


def test_per_instance_mu():
    nb = 24
    mu = np.linspace(0.3, 1.4, nb).astype(np.float32)

    def setup(mpc):
        d_mu = sc.torch_().from_numpy(mu).cuda()
        mpc.set_instance_mu(d_mu.data_ptr(), keepalive=d_mu)
        return d_mu

    assert_on_equals_off(standing(nb, seed=386), 10, setup=setup)


def test_non_default_parameters():
    assert_on_equals_off(standing(24, seed=387), 10, setup=lambda mpc: mpc.set_params(**fc.PARAM_SET_0))


def test_the_smallest_batch_with_a_dispatch_order():
    """513 instances: workgroup b of the solve no longer takes instance b, the prologue's blocks stay indexed by instance."""
    assert_on_equals_off(standing(513, seed=388), 10)


@pytest.mark.parametrize("gait,h", [("standing", 10), ("walking", 10), ("single", 20)])
def test_device_repair_on_the_3x_rows(gait, h):
    """A continuation that resumes re-assembles in the kernel: it must agree with the prologue's assembly of the fast pass."""
    rec = records.pack_records(synthetic.hard_batch(64, h, gait, 17, 3), h)
    assert_on_equals_off(rec, h, setup=lambda mpc: mpc.set_device_repair(True))


def test_one_tick_built_and_solved_on_the_device():
    """hmpc_tick_solve_device: the record builder and the prologue on one stream."""
    torch = sc.torch_()
    nb, h = 40, 10
    t = synthetic.make_ticks(nb, h, "walking", seed=389)
    out = {}
    for on in (True, False):
        mpc = interface.BatchedMPC(DT, h, FMAX, nb)
        mpc.debug_set_front_prologue(on)
        d_t = torch.from_numpy(np.ascontiguousarray(t).view(np.uint8).reshape(len(t), -1).copy()).cuda()
        d_tau = torch.zeros((nb, 10), dtype=torch.float64, device="cuda")
        d_ff = torch.zeros((nb, 12), dtype=torch.float64, device="cuda")
        mpc.tick_solve_device(d_t.data_ptr(), nb, DT, d_tau.data_ptr(), d_ff.data_ptr(), 0, 0)
        forces, status = mpc.download()
        out[on] = dict(forces=forces, status=status, tau=d_tau.cpu().numpy(), f_ff=d_ff.cpu().numpy())
        mpc.close()
    sc.assert_same(out[True], out[False], "tick on against off")
    assert np.abs(out[True]["tau"]).max() > 0.1


# ------------------------------------------------------------------------------------------------ (c)
def test_a_second_batch_on_a_busy_stream_equals_a_fresh_handle():
    torch = sc.torch_()
    h = 10
    rec_a, rec_b = standing(64, seed=390), records.pack_records(synthetic.make_batch(17, h, "walking", seed=391, phase="random"), h)
    fresh = interface.BatchedMPC(DT, h, FMAX, 64)
    d_b = torch.from_numpy(rec_b).cuda()
    fresh.set_device_records(d_b.data_ptr(), 17, keepalive=d_b)
    fresh.solve()
    want = dict(zip(("forces", "status"), fresh.download()))
    fresh.close()
    mpc = interface.BatchedMPC(DT, h, FMAX, 64)
    mpc.upload(rec_a)
    mpc.solve()
    mpc.download()
    busy = sc.Busy().hold()
    mpc.set_device_records(d_b.data_ptr(), 17, keepalive=d_b)
    mpc.solve(busy.s)
    busy.still_held("solve of the second batch")
    busy.wait()
    got = dict(zip(("forces", "status"), mpc.download()))
    mpc.close()
    sc.assert_same(got, want, "second batch on a busy stream")
