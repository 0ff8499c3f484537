"""CPU-only checks of the 1- and 2-link arm surface: default_config(..., n_joints=k) cuts the default arm to its first k links (their masses
leave vehicle.mass, as tests/test_gpu_arm.py builds the vehicle), the C ABI reports the caller's dimensions, the PPO fused paths are
declared for those dimensions, and the header documents them."""
import os
import re

import pytest

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd import _lib as L
from rl_aerial_manipulator_amd.ppo import ActorCritic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK_MASS = [0.082, 0.054, 0.220]   # the default arm's links (amenv_capi.hip vehicle_hexa_arm)


@pytest.mark.parametrize("nj", [1, 2, 3])
def test_default_config_cuts_the_arm(nj):
    full = L.default_config("hexa_arm", 64)
    cfg = L.default_config("hexa_arm", 64, n_joints=nj)
    assert cfg.vehicle.n_joints == nj and cfg.num_envs == 64
    assert list(full.vehicle.link_mass[:3]) == LINK_MASS
    assert cfg.vehicle.mass == full.vehicle.mass - sum(LINK_MASS[nj:])
    assert cfg.task.ee_task == L.EE_TASK_TOOL
    if nj < 3:
        assert cfg.vehicle.mass < full.vehicle.mass


@pytest.mark.parametrize("nj,dims", [(1, (25, 5)), (2, (27, 6)), (3, (29, 7))])
def test_dims_of_the_shorter_arms(nj, dims):
    import ctypes as C
    cfg = L.default_config("hexa_arm", 16, n_joints=nj)
    od, ad = C.c_int32(), C.c_int32()
    assert L.load().amenv_dims(C.byref(cfg), C.byref(od), C.byref(ad), None, None) == 0
    assert (od.value, ad.value) == dims
    assert dims in ActorCritic._FUSED_DIMS


def test_n_joints_needs_the_arm_vehicle():
    for vehicle in ("quad", "hexa"):
        with pytest.raises(amd.AmenvError, match="n_joints"):
            L.default_config(vehicle, 8, n_joints=1)
    for nj in (0, 4):
        with pytest.raises(amd.AmenvError, match="n_joints"):
            L.default_config("hexa_arm", 8, n_joints=nj)
    with pytest.raises(amd.AmenvError, match="n_joints"):
        amd.GpuWaypointEnv(8, vehicle="hexa", n_joints=2)        # refused before any device is touched


def test_header_documents_act_dim_5_and_6():
    hdr = open(os.path.join(ROOT, "include", "amenv.h")).read()

    def comment_before(fn):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:size_t amenv_\w+\(void\);\s*)?int " + fn + r"\(", hdr, re.S)
        assert m, fn
        return m.group(1)

    for fn in ("amenv_gaussian_act", "amenv_ppo_loss_grad"):
        assert re.search(r"act_dim[^.]*\b5\b[^.]*\b6\b", comment_before(fn)), fn
    for fn in ("amenv_policy_forward", "amenv_ppo_mlp_step"):
        c = comment_before(fn)
        assert "(25,5)" in c.replace(" ", "") and "(27,6)" in c.replace(" ", ""), fn
