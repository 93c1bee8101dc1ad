"""GPU parity of the assembly chains (stage_a_chains of csrc/hmpc_kernel.h over csrc/hmpc_chains.h: the powers of Acd as fourteen recurrences in
registers, Phi_k and e in one pass behind them) at the shapes where the loop structure can go wrong: the smallest horizon the handle accepts
(a power phase of one step, a block of the item phase with one live step), h = 2 and 3, the wide variant's first horizon (h = 11: three blocks
of the item phase, the last with one live step, on 512 threads), three contacts (234 Phi items: the e items are a second trip of wave 0) at the
smallest horizon and at h = 10.  (Horizons of up to three steps run on the 60-variable kernels, 128 threads and two trips of items.)  H, g, x0, Acd, Bcd of debug_assemble BIT-IDENTICAL to the oracle's, as in tests/test_gpu_assembly.py; g carries every
Phi_k and every e_k, H every Phi_k.  tests/test_chains_on_host.py checks the header's arithmetic without a GPU."""
import numpy as np
import pytest

from hector_simulation_amd import interface, records, synthetic

pytestmark = pytest.mark.gpu

NB = 4
CASES = [("standing", 1, 2, 381), ("walking", 1, 2, 382), ("standing", 2, 2, 383), ("walking", 2, 2, 384), ("standing", 3, 2, 385),
         ("walking", 3, 2, 386), ("standing", 11, 2, 387), ("standing", 1, 3, 388), ("standing", 10, 3, 389)]


@pytest.mark.parametrize("gait,h,nc,seed", CASES)
def test_chains_bitwise(oracle, gait, h, nc, seed):
    if nc == 3:
        f = synthetic.make_batch3(NB, h, gait, seed=seed, hand="contact", phase="random")
    else:
        f = synthetic.make_batch(NB, h, gait, seed=seed, phase="random", yaw_rate_cmd=True)
    rec = records.pack_records(f, h, nc)
    mpc = interface.BatchedMPC(synthetic.DT_MPC, h, synthetic.F_MAX, NB, contacts=nc)
    mpc.upload(rec)
    try:
        for k in range(NB):
            o = oracle.assemble_record(rec[k], h, synthetic.DT_MPC, synthetic.F_MAX, nc=nc)
            d = mpc.debug_assemble(k)
            assert d["n"] == o["n"] and d["m"] == o["m"] and d["n"] > 0
            for name in ("x0", "Acd", "Bcd"):
                np.testing.assert_array_equal(d[name].view(np.uint32), o[name].view(np.uint32), err_msg=name)
            Ho, go = o["H_red"].astype(np.float32), o["g_red"].astype(np.float32)
            assert np.array_equal(Ho.astype(np.float64), o["H_red"]) and np.array_equal(go.astype(np.float64), o["g_red"])  # widened floats
            np.testing.assert_array_equal(d["g"].view(np.uint32), go.view(np.uint32), err_msg="g")
            np.testing.assert_array_equal(d["H"].view(np.uint32), Ho.view(np.uint32), err_msg="H")
    finally:
        mpc.close()
