"""tests/switch_harness.py without a GPU: its data are, bit for bit, what the five switch test files each built for themselves before they
shared it (recorded from those definitions into tests/golden/switch_harness.npz), and its comparisons fail when one element of one compared
field differs -- a helper that compares nothing cannot pass this file."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd import _lib as L
from tests import switch_harness as H

GOLD = np.load(os.path.join(H.GOLD, "switch_harness.npz"))
N = 4
DONE = [0, 1, 0, 1]


# ---- the data ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n,seed", [(3, 5, 1), (2, 200, 4)])
@pytest.mark.parametrize("kind,kw", [("plain", {}), ("wide", dict(wide=True)), ("tipped", dict(tipped=True))])
def test_actions_are_the_recorded_ones(T, n, seed, kind, kw):
    """plain / wide: the randomisation, lag and delay files' generator (wide: also the history file's); tipped: the noise file's."""
    got = H.actions(T, n, seed, "cpu", **kw)
    want = GOLD[f"actions_{T}_{n}_{seed}_{kind}"]
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (T, n, 4) == want.shape
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(want, GOLD[f"actions_{T}_{n}_{seed}_{'wide' if kind == 'plain' else 'plain'}"])


def _flatten(s, prefix=""):
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            out.update(_flatten(v, prefix + name + "."))
        else:
            out[prefix + name] = np.array(list(v) if isinstance(v, C.Array) else v)
    return out


@pytest.mark.parametrize("gid0", [0, 1000])
def test_octo_config_is_the_recorded_one(gid0):
    """Field by field against the three earlier copies (they differed in env_id_offset alone: 0 in the noise file, 1000 in the other two).
    Exact, except `alloc`: a pseudo-inverse, whose last bits belong to the LAPACK at hand -- exact against the pseudo-inverse of the
    recorded `mix` taken here, and within 1e-12 of the recorded one."""
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libamenv.so is not built: no default_config")
    got = _flatten(H.octo_config(64, gid0))
    keys = sorted(k[5:] for k in GOLD.files if k.startswith("octo."))
    assert sorted(got) == keys and len(keys) > 20
    for k in keys:
        want = GOLD["octo." + k]
        if k == "env_id_offset":
            assert got[k] == gid0 and want == 0
        elif k == "vehicle.alloc":
            mix = GOLD["octo.vehicle.mix"].reshape(4, L.MAX_ROTORS)[:, :8]
            assert np.array_equal(got[k].reshape(L.MAX_ROTORS, 4)[:8], np.linalg.pinv(mix))
            np.testing.assert_allclose(got[k], want, rtol=1e-12, atol=1e-15)
        else:
            assert got[k].dtype == want.dtype and np.array_equal(got[k], want), k
    assert got["vehicle.n_rotors"] == 8 and got["num_envs"] == 64


def test_buffers_and_all_written():
    z, nan = H.buffers(3, N, 5, "cpu"), H.buffers(3, N, 5, "cpu", fill=float("nan"))
    assert {k: (tuple(v.shape), v.dtype) for k, v in z.items()} == {k: (tuple(v.shape), v.dtype) for k, v in nan.items()}
    assert z["obs"].shape == (4, N, 5) and z["actions"].shape == (3, N, 4) and z["dones"].dtype == torch.uint8 and z["logp"].dtype == torch.float32
    assert all(not bool(v.any()) for v in z.values())
    assert all(bool(torch.isnan(v).all()) for k, v in nan.items() if k != "dones") and bool((nan["dones"] == 0xFF).all())
    H.all_written(z)
    for k in nan:
        part = {j: (v if j == k else z[j]) for j, v in nan.items()}       # one buffer left unwritten
        with pytest.raises(AssertionError):
            H.all_written(part)
        one = {j: v.clone() for j, v in z.items()}
        one[k].view(-1)[7] = nan[k].view(-1)[7]                               # one entry left unwritten
        with pytest.raises(AssertionError):
            H.all_written(one)


# ---- the comparisons --------------------------------------------------------------------------------------------------------------
class Stub:
    """The surface the comparisons read, on the CPU: 4 envs, envs 1 and 3 end in the step."""
    def __init__(self):
        g = torch.Generator().manual_seed(1)
        self.obs, self.reward = torch.rand(N, 6, generator=g), torch.rand(N, generator=g)
        self.done, self.info_bits = torch.tensor(DONE, dtype=torch.uint8), torch.tensor([0, 5, 0, 9], dtype=torch.int32)
        self.terminal_obs, self.ep_return, self.ep_len = torch.rand(N, 6, generator=g), torch.rand(N, generator=g), torch.tensor([3, 7, 2, 9], dtype=torch.int32)
        self.fstate, self.istate = torch.rand(13, N, generator=g), torch.arange(4 * N, dtype=torch.int32).reshape(4, N)
        self.w = torch.rand(N, 4, generator=g)

    def step(self, a):
        return self.obs, self.reward, self.done, self.info_bits

    def get_state(self):
        return self.fstate.clone(), self.istate.clone()

    def rotor_state(self):
        return self.w.clone()


STEP_FIELDS = ["obs", "reward", "done", "info_bits", "terminal_obs", "ep_return", "ep_len"]


def _bump(t, env):
    """One element of env's row changes."""
    flat = t[env].reshape(-1) if t.dim() > 1 else t[env:env + 1]
    flat[-1] = flat[-1] + 1 if t.dtype != torch.uint8 else 1 - flat[-1]


def test_comparisons_pass_on_equal_inputs():
    a, b = Stub(), Stub()
    ra, da = H.step_all(a, None); rb, db = H.step_all(b, None)
    assert len(ra) == 7 and all(x is not getattr(a, k) and torch.equal(x, getattr(a, k)) for x, k in zip(ra, STEP_FIELDS)) and da.tolist() == [False, True, False, True]
    H.same_step(ra, da, rb, db, 0)
    H.same_state(a, b)
    H.same_outputs(dict(obs=a.obs, done=a.done), dict(obs=b.obs, done=b.done))
    H.ROTOR_LAG.same_side_state(a, b)


@pytest.mark.parametrize("field", STEP_FIELDS)
@pytest.mark.parametrize("env", range(N))
def test_same_step_sees_one_element(field, env):
    """obs, reward, done, info at every env; terminal_obs, ep_return, ep_len where the env ended, and only there (undefined elsewhere)."""
    a, b = Stub(), Stub()
    _bump(getattr(b, field), env)
    ra, da = H.step_all(a, None); rb, db = H.step_all(b, None)
    if field in STEP_FIELDS[:4] or DONE[env]:
        with pytest.raises(AssertionError):
            H.same_step(ra, da, rb, db, 0)
        with pytest.raises(AssertionError):
            H.same_step(rb, db, ra, da, 0)
    else:
        H.same_step(ra, da, rb, db, 0)


@pytest.mark.parametrize("field", ["fstate", "istate", "w"])
def test_same_state_and_side_state_see_one_element(field):
    a, b = Stub(), Stub()
    t = getattr(b, field)
    t[-1, 2] = t[-1, 2] + 1
    check = (lambda: H.ROTOR_LAG.same_side_state(a, b)) if field == "w" else (lambda: H.same_state(a, b))
    with pytest.raises(AssertionError):
        check()
    (H.same_state if field == "w" else H.ROTOR_LAG.same_side_state)(a, b)     # and the other comparison does not look there


def test_same_outputs_sees_one_element_and_a_missing_key():
    a, b = Stub(), Stub()
    da, db = dict(obs=a.obs, reward=a.reward), dict(obs=b.obs, reward=b.reward)
    H.same_outputs(da, db)
    _bump(b.reward, 3)
    with pytest.raises(AssertionError):
        H.same_outputs(da, db)
    with pytest.raises(AssertionError):
        H.same_outputs(dict(obs=a.obs), dict(obs=b.obs, reward=a.reward))
    with pytest.raises(AssertionError):
        H.same_outputs({}, {})


def test_the_descriptors():
    sw = [H.RANDOMIZATION, H.ROTOR_LAG, H.SENSOR_NOISE, H.ACTION_DELAY, H.ACTION_HISTORY]
    assert [s.suffix for s in sw] == ["+dr", "+lag", "+noise", "+delay", "+history"]
    assert all(s.setter == "set_" + s.kw for s in sw)
    assert all(callable(getattr(amd.GpuWaypointEnv, s.setter)) for s in sw)
