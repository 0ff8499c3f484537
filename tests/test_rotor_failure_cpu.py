"""Per-episode rotor failure, host side (no GPU; include/amenv.h amenv_set_rotor_failure): RotorFailure's checks and
C layout, the numpy restatement of the draw (tests/fail_ref.py) at its edges and on recorded plans, the declared and exported entry
points, and the condition of the GPU oracle gate -- enough steps before and behind the onset -- from the restatement alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rl_aerial_manipulator_amd as amd
from rl_aerial_manipulator_amd.gpu_env import _SWITCHES
from tests import dr_ref, fail_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the Python class -------------------------------------------------------------------------------------------------------------
def test_rotor_failure_values_refused():
    nan, inf = float("nan"), float("inf")
    for bad in (nan, inf, -0.1, 1.1, "1", None, True):
        with pytest.raises(amd.AmenvError, match="RotorFailure"):
            amd.RotorFailure(probability=bad)
    for bad in ((-1, 5), (6, 5), (0, 65536), (0.5, 3), (1, 2.0), (1,), 3, (1, 2, 3), (None, 2), (True, 2)):
        with pytest.raises(amd.AmenvError, match="RotorFailure"):
            amd.RotorFailure(onset=bad)
    for bad in ((-0.1, 0.5), (0.6, 0.5), (0.0, 1.1), (nan, 0.5), (0.0, inf), (0.5,), 0.5, ("0", 1)):
        with pytest.raises(amd.AmenvError, match="RotorFailure"):
            amd.RotorFailure(remaining=bad)
    for bad in ([], [-1], [8], [0, 0], [0.0], [True], 2, ["1"]):
        with pytest.raises(amd.AmenvError, match="RotorFailure"):
            amd.RotorFailure(rotors=bad)
    amd.RotorFailure(rotors=[5]).validate(6)
    with pytest.raises(amd.AmenvError, match="4 rotors"):   # checked against the env when it is set
        amd.RotorFailure(rotors=[1, 5]).validate(4)
    with pytest.raises(amd.AmenvError, match="RotorFailure"):   # the wrong type, before any device is touched
        amd.GpuWaypointEnv(8, rotor_failure=0.5)


def test_rotor_failure_accepted_and_packed():
    r = amd.RotorFailure()
    assert (r.probability, r.onset, r.remaining, r.rotors, r.rotor_mask) == (1.0, (0, 0), (0.0, 0.0), None, 0)
    r = amd.RotorFailure(probability=np.float32(0.25), onset=(np.int64(3), 65535), remaining=(0, np.float64(0.5)), rotors=(4, 0, 2))
    assert repr(r) == "RotorFailure(probability=0.25, onset=(3, 65535), remaining=(0.0, 0.5), rotors=(0, 2, 4))"
    c = r.to_c()
    assert (c.struct_size, c.probability, c.onset_min, c.onset_max, c.remaining_min, c.remaining_max, c.rotor_mask) == (28, 0.25, 3, 65535, 0.0, 0.5, 0b10101)


def test_struct_matches_the_header_and_symbols_are_exported():
    """The ctypes struct has the header's fields in the header's order, all 4 bytes wide: its size is the header's."""
    hdr = open(os.path.join(ROOT, "include", "amenv.h")).read()
    body = re.search(r"typedef struct amenv_rotor_failure \{(.*?)\} amenv_rotor_failure;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    types = [decl.strip().split(None, 1)[0] for decl in body.split(";") if decl.strip()]
    K = amd._lib.RotorFailureC
    assert names == [f[0] for f in K._fields_] == ["struct_size", "probability", "onset_min", "onset_max", "remaining_min", "remaining_max", "rotor_mask"]
    assert set(types) <= {"uint32_t", "int32_t", "float"}
    assert C.sizeof(K) == 4 * len(names) == 28 and all(getattr(K, n).size == 4 for n in names)
    lib = amd._lib.load()
    for name in ("amenv_set_rotor_failure", "amenv_rotor_failure_state"):
        assert name in amd._lib.SYMBOLS and hasattr(lib, name) and f"int {name}(" in hdr
    assert "RotorFailure" in amd.__all__ and "rotor_failure" in _SWITCHES
    bad = amd.RotorFailure().to_c()      # a NULL handle is refused before anything is read
    assert lib.amenv_set_rotor_failure(None, C.byref(bad)) == -1 and lib.amenv_rotor_failure_state(None, None, None, None) == -1


# ---- 2. the restatement ----------------------------------------------------------------------------------------------------------------
PAIRS = [(gid, ep) for gid in list(range(60)) + [2 ** 31 - 1, 2 ** 31, 2 ** 32 + 5, 2 ** 40] for ep in range(1, 65)]   # 4,096 (gid, episode) pairs


def test_probability_edges_mask_and_ranges():
    assert len(PAIRS) == 4096
    assert fail_ref.p16(0.0) == 0 and fail_ref.p16(1.0) == 65536 and fail_ref.p16(0.5) == 32768 and fail_ref.p16(1e-6) == 0 and fail_ref.p16(0.99999) == 65535
    never = amd.RotorFailure(probability=0.0, onset=(3, 9), remaining=(0.0, 0.5))
    always = amd.RotorFailure(probability=1.0, onset=(3, 9), remaining=(0.25, 0.5), rotors=[0, 3, 4, 5])
    half = amd.RotorFailure(probability=0.5, onset=(0, 65535), remaining=(0.0, 1.0))
    rotors, onsets, fs, hits = set(), set(), [], 0
    for gid, ep in PAIRS:
        assert fail_ref.plan(7, gid, ep, 6, never)[:2] == (-1, 0)
        r, o, f = fail_ref.plan(7, gid, ep, 6, always)
        assert r in (0, 3, 4, 5) and 3 <= o <= 9 and np.float32(0.25) <= f <= np.float32(0.5) and f.dtype == np.float32
        rotors.add(r); onsets.add(o); fs.append(f)
        r, o, f = fail_ref.plan(7, gid, ep, 4, half)
        assert (r == -1 and o == 0) or (0 <= r < 4 and 0 <= o <= 65535)
        assert 0.0 <= f <= 1.0
        hits += r >= 0
    assert rotors == {0, 3, 4, 5} and onsets == set(range(3, 10)) and len(set(fs)) > 2000
    assert abs(hits - 2048) < 4 * 32          # binomial(4096, 1/2): sigma = 32
    # the same halves drive every field: the rotor does not depend on the onset range, nor the onset on the mask
    for gid, ep in PAIRS[:64]:
        a = fail_ref.plan(7, gid, ep, 6, always)
        b = fail_ref.plan(7, gid, ep, 6, amd.RotorFailure(probability=1.0, onset=(0, 100), remaining=(0.25, 0.5), rotors=[0, 3, 4, 5]))
        c = fail_ref.plan(7, gid, ep, 6, amd.RotorFailure(probability=1.0, onset=(3, 9), remaining=(0.25, 0.5)))
        assert a[0] == b[0] and a[1] == c[1] and a[2] == b[2] == c[2]


def test_effective_flips_at_the_onset():
    pl = (2, 5, np.float32(0.375))
    for step in range(0, 5):
        assert np.array_equal(fail_ref.effective(pl, step, 6), np.ones(6, np.float32))
    for step in (5, 6, 65535, 10 ** 6):
        assert np.array_equal(fail_ref.effective(pl, step, 6), np.float32([1, 1, 0.375, 1, 1, 1]))
    assert np.array_equal(fail_ref.effective((-1, 0, np.float32(0.375)), 3, 4), np.ones(4, np.float32))
    assert np.array_equal(fail_ref.effective((0, 0, np.float32(0.0)), 0, 4), np.float32([0, 1, 1, 1]))


# (rotor, onset, f as a hex float) of the five keys of test_recorded_plans; the halves of the second are (8829, 25789, 51941, 3185):
# 8829 < 49152, (25789 * 4) >> 16 = 1 -> rotor 2 of [1, 2, 4, 5], 3 + ((51941 * 398) >> 16) = 318, 0.1 + 0.5 * (3185 * 2^-16)
RECORDED = [(-1, 0, "0x1.8018cc0000000p-3"), (2, 318, "0x1.fd219a0000000p-4"), (4, 381, "0x1.1ed9340000000p-1"), (4, 283, "0x1.69c4cc0000000p-3"),
            (-1, 0, "0x1.f5e2660000000p-2")]


def test_recorded_plans():
    """Five plans as literals: they pin the restatement itself (the Philox block index, the cut of the halves, the integer products, the
    fp32 arithmetic), which the GPU test then holds the device function to."""
    p = amd.RotorFailure(probability=0.75, onset=(3, 400), remaining=(0.1, 0.6), rotors=[1, 2, 4, 5])
    got = [fail_ref.plan(seed, gid, ep, 6, p) for seed, gid, ep in [(0, 0, 1), (8, 63, 2), (21, 511, 7), (2 ** 40 + 3, 2 ** 33 + 1, 1), (13, 100, 300)]]
    assert [(r, o, float(f).hex()) for r, o, f in got] == RECORDED


def test_oracle_config_scales_the_mixer_columns():
    from oracle import oracle as O
    base = O.Config.from_buffer_copy(amd._lib.default_config("hexa", 4))
    dr = np.float32([1.25, 0.8, 0.9, 1.1, 1.0, 0.95, 1.05, 1.0])
    ff = np.float32([1, 1, 0.3, 1, 1, 1])
    for dtype in ("f32", "f64"):
        out = fail_ref.oracle_config(base, dr, ff, gid=3, dtype=dtype)
        ref = dr_ref.oracle_config(base, dr, gid=3)
        assert out.num_envs == 1 and out.env_id_offset == 3
        s2 = np.float64(np.float32(1.0) * np.float32(0.3)) if dtype == "f32" else np.float64(np.float32(1.0)) * np.float64(np.float32(0.3))
        for r in range(6):
            for i in range(4):
                want = ref.vehicle.mix[i * 6 + r] if r != 2 else base.vehicle.mix[i * 6 + r] * s2 / (1.25 if i == 0 else 1.0)
                assert out.vehicle.mix[i * 6 + r] == want, (dtype, r, i)
        assert list(out.vehicle.inertia) == list(ref.vehicle.inertia)


# ---- 3. the oracle gate's condition ----------------------------------------------------------------------------------------------------
def test_oracle_gate_runs_on_both_sides_of_the_onset():
    """tests/test_gpu_rotor_failure.py's oracle case: probability 1, onset (3, 9), max_episode_steps = 12, so an episode that runs into
    the time limit takes 13 calls (step fields 0..12).  Over the 64 envs' first three episodes at seed 8, at least 25 % of the (env, step)
    pairs lie before their onset and at least 25 % behind it, whatever ends an episode earlier shifts weight to `before` only: the GPU
    test asserts both shares on the steps it actually ran."""
    p = amd.RotorFailure(probability=1.0, onset=(3, 9), remaining=(0.0, 0.5))
    before = after = 0
    for gid in range(64):
        for ep in (1, 2, 3):
            r, o, f = fail_ref.plan(8, gid, ep, 4, p)
            assert r >= 0
            before += o; after += 13 - o
    share = before / (before + after)
    print(f"before the onset: {share:.3f}, behind it: {1 - share:.3f}")
    assert share >= 0.25 and 1 - share >= 0.25
    assert abs(share - 6 / 13) < 0.05
