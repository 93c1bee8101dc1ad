"""Every kernel launched behind a solve, at every arm of the shape rule and its edges (csrc/hmpc_derived_shape.h): (contacts, horizon) =
(2, 1), (2, 10), (2, 11), (2, 20), (3, 10).

What the kernels share before their own arithmetic (csrc/hmpc_derived.h) is the part that knows about the batch: the offset of the
instance's record, the offset of its slot of the force buffer, the guard, and, in the two tiled launches, the offsets of a tile's seeds
and outputs.  So a batch of three distinct records -- standing, walking at phase 0, walking mid-gait: different gait bytes -- is solved
and every family requested behind it; then each record alone goes through a second handle of batch 1 that sees the same force bytes, and
every array of instance k of the batch must equal the lone handle's bytewise.  The multi-seed adjoint and the chain run 6 contacts + 1
seeds: a second tile of one seed."""
import numpy as np
import pytest

from hector_simulation_amd import interface, records, synthetic

pytestmark = pytest.mark.gpu
SHAPES = [(2, 1), (2, 10), (2, 11), (2, 20), (3, 10)]
NB = 3


def three_records(nc, h):
    """(records, the same robots a tick later) of a standing instance, a walking one at phase 0 and a walking one mid-gait."""
    make = synthetic.make_batch if nc == 2 else synthetic.make_batch3
    parts = [make(1, h, "standing", seed=380 + h), make(1, h, "walking", seed=381 + h, phase=0),
             make(1, h, "walking", seed=382 + h, phase=h // 2 + h // 4, **({"hand": "window"} if nc == 3 else {}))]
    f = {k: np.concatenate([np.asarray(p[k]) for p in parts]) for k in parts[0]}
    rec = records.pack_records(f, h, nc)
    rec2 = records.pack_records(synthetic.advance_tick(f, h, seed=38), h, nc)
    return rec, rec2


def everything_behind(mpc, rec2, ell, seeds):
    """Every derived family of a solved handle, downloaded: {family: {array: (values, axis of the instance)}}."""
    from test_gpu_adjoint import _device
    from test_gpu_adjoint_chain import device_buffers, give
    from test_gpu_pose_adjoint import chain_with

    nb, S = ell.shape[0], seeds.shape[0]
    out = {}
    mpc.predict_states()
    states, cost = mpc.download_prediction()
    out["prediction"] = dict(states=states, cost=cost)
    mpc.constraint_margins()
    out["margins"] = mpc.download_margins()
    mpc.kkt_certificate()
    out["certificate"] = mpc.download_certificate()
    mpc.feedback_gains()
    out["gains"] = mpc.download_gains()
    t_new = _device(rec2)
    mpc.first_order_wrench(t_new.data_ptr())
    out["first_order"] = mpc.download_first_order()
    out["adjoint"], out["adjoint_model"], out["adjoint_limits"], out["adjoint_record"] = chain_with(mpc, ell)
    t_seeds = _device(seeds)
    mpc.solve_adjoint_multi(t_seeds.data_ptr(), S)
    multi = mpc.download_adjoint_multi()
    give(mpc, S, device_buffers(S, nb, mpc.horizon, mpc.contacts))
    mpc.adjoint_chain_multi(t_seeds.data_ptr())
    chain = mpc.download_adjoint_chain_multi(detail=True)
    res = {fam: {k: (v, 0) for k, v in arrays.items()} for fam, arrays in out.items()}
    res["adjoint_multi"] = {k: (v, 1) for k, v in multi.items()}          # [seed, instance, ...]
    res["adjoint_chain_multi"] = {k: (v, 1) for k, v in chain.items()}
    return res


def solved_alone(rec_k, h, nc, forces_k):
    """A handle of batch 1 with record k solved, seeing the force bytes ``forces_k`` the batch's solve left for it (a batch of three runs
    on the variant of its widest instance, so the lone solve may round differently: then the batch's forces are written into the lone
    handle's own output buffer).  Returns (handle, whether the lone solve's forces were the batch's already)."""
    import torch

    t_f = torch.zeros((1, 6 * nc * h), dtype=torch.float32, device="cuda")
    t_s = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, 1, contacts=nc)
    mpc.set_device_outputs(t_f.data_ptr(), t_s.data_ptr(), keepalive=(t_f, t_s))
    mpc.upload(rec_k[None])
    mpc.solve()
    own, _ = mpc.download()
    same = np.array_equal(own.view(np.uint32), forces_k[None].view(np.uint32))
    if not same:
        t_f.copy_(torch.from_numpy(np.ascontiguousarray(forces_k[None])))
        torch.cuda.synchronize()
    seen, _ = mpc.download()
    np.testing.assert_array_equal(seen.view(np.uint32), forces_k[None].view(np.uint32))   # first: the same force bytes
    return mpc, same


def bytes_of(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


@pytest.mark.parametrize("nc,h", SHAPES, ids=[f"c{nc}_h{h}" for nc, h in SHAPES])
def test_every_family_of_instance_k_is_what_record_k_alone_gives(nc, h):
    U, S = 6 * nc, 6 * nc + 1
    rec, rec2 = three_records(nc, h)
    gait = np.asarray(records.unpack_records(rec, h, nc)["gait"]).reshape(NB, -1)
    assert len({g.tobytes() for g in gait}) > 1 and len({r.tobytes() for r in rec}) == NB
    rng = np.random.default_rng(3800 + 10 * h + nc)
    ell = rng.standard_normal((NB, h, U))
    seeds = rng.standard_normal((S, NB, h, U))
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, NB, contacts=nc)
    mpc.upload(rec)
    mpc.solve()
    forces, status = mpc.download()
    assert (interface.status_code(status) == 0).all(), status
    batch = everything_behind(mpc, rec2, ell, seeds)
    mpc.close()
    assert batch["adjoint_multi"]["dir"][0].shape == (S, NB, h, U) and batch["adjoint_chain_multi"]["grad_record"][0].shape[:2] == (S, NB)
    # (the instances differ, so that an offset of the wrong instance cannot pass)
    assert len({bytes_of(batch["prediction"]["states"][0][k]).tobytes() for k in range(NB)}) == NB
    assert np.abs(batch["adjoint_chain_multi"]["grad_record"][0][S - 1]).max() > 0   # the second tile's one seed
    different, already = [], []
    for k in range(NB):
        solo, same = solved_alone(rec[k], h, nc, forces[k])
        already.append(same)
        alone = everything_behind(solo, rec2[k:k + 1], np.ascontiguousarray(ell[k:k + 1]), np.ascontiguousarray(seeds[:, k:k + 1]))
        solo.close()
        assert alone.keys() == batch.keys()
        for fam, arrays in batch.items():
            assert arrays.keys() == alone[fam].keys(), fam
            for key, (v, axis) in arrays.items():
                if not np.array_equal(bytes_of(np.take(v, k, axis=axis)), bytes_of(np.take(alone[fam][key][0], 0, axis=axis))):
                    different.append((k, fam, key))
    print(f"c{nc} h{h}: lone solve gave the batch's force bytes for instances {already}; arrays compared per instance "
          f"{sum(len(a) for a in batch.values())}; different {different}")
    assert not different, different
