"""examples/best_command.c (a command sweep, the prediction, then the best command of every state picked on the device) compiled against
include/hector_mpc.h and linked to the in-tree library, on the pattern of tests/test_prediction_example.py: without a GPU it must fail
loudly, with one it must run; and the new entry points refuse a NULL handle without touching a device."""
import ctypes as C
import subprocess

import pytest

from hector_simulation_amd import _lib, interface
from test_examples import _compile, _has_gpu

SRC = ("best_command.c", "gcc", "-std=c11")


def test_selection_example_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    if _has_gpu():
        pytest.skip("GPU present: covered by the gpu-marked test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "no HIP device" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_selection_example_runs_on_gpu(tmp_path):
    exe = _compile(tmp_path, *SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "best command of 3 states x 8 commands: 0 problems" in r.stdout
    assert r.stdout.count("chosen command") == 3 and r.stdout.count("predicted vx at step 10") == 3


def test_new_entry_points_refuse_a_null_handle():
    L = _lib.load()
    assert L.hmpc_sweep_select(None, 4, None, None) == -1  # HMPC_E_ARG
    assert L.hmpc_set_device_selection(None, None, None, None, None, None) == -1
    g = C.c_int(7)
    assert L.hmpc_get_device_selection(None, None, None, None, None, None, C.byref(g)) == -1
    assert L.hmpc_download_selection(None, None, None, None, None, None) == -1
    assert L.hmpc_tick_sweep_device(None, None, 1, None, 1, 0.04, None, None, None, None, None) == -1


def test_command_struct_is_forty_bytes(tmp_path):
    """sizeof(struct hmpc_command) as a C compiler lays it out == COMMAND_DTYPE == the ctypes mirror: five doubles, the command fields of
    hmpc_tick_inputs in their order."""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hector_mpc.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(struct hmpc_command), offsetof(struct hmpc_command, yaw_rate_des), offsetof(struct hmpc_command, roll_des), "
                   "offsetof(struct hmpc_command, pitch_des), offsetof(struct hmpc_tick_inputs, world_position_desired) - "
                   "offsetof(struct hmpc_tick_inputs, v_des_robot)); return 0; }\n")
    exe = str(tmp_path / "size")
    import os

    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-std=c11", "-I" + inc, str(src), "-o", exe], check=True)
    size, o_yaw, o_roll, o_pitch, span = (int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert size == 40 == interface.COMMAND_DTYPE.itemsize == C.sizeof(_lib.Command) == span
    f = interface.COMMAND_DTYPE.fields
    assert (o_yaw, o_roll, o_pitch) == (f["yaw_rate_des"][1], f["roll_des"][1], f["pitch_des"][1]) == (16, 24, 32)
    t = interface.TICK_DTYPE.fields
    assert t["pitch_des"][1] - t["v_des_robot"][1] == 32 and t["world_position_desired"][1] - t["v_des_robot"][1] == 40
