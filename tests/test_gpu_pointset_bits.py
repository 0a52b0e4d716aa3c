"""hint_hausdorff_run, hint_plus_run, hint_lensfit_run and hint_plusfit_run give, on the cases of tests/pointset_cases.py, the bits
that tests/golden/pointset_bits.npz recorded before each kernel was built from the shared core (hint_amd/csrc/hint_pointset.hpp)
and tests/golden/plusfit_bits.npz before the two fits were built on one driver (hint_amd/csrc/hint_fit.hpp): every output compared
as int32 words, exactly.  A generator that drifted is told apart from a kernel that did: the fixture holds
a sha256 of every input."""
import os

import numpy as np
import pytest

import pointset_cases as pc

pytestmark = pytest.mark.gpu

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointset_bits.npz")
GOLD = np.load(PATH)
NAMES = list(pc.HAUSDORFF) + list(pc.PLUS) + list(pc.LENSFIT)
PF_PATH = os.path.join(os.path.dirname(PATH), "plusfit_bits.npz")
PF_GOLD = np.load(PF_PATH)
QNAN = 0x7fc00000


def test_the_fixture_holds_every_case_and_is_small():
    assert {k.split("/")[0] for k in GOLD.files} == set(NAMES) | {"build"}
    assert os.path.getsize(PATH) < 64 << 10
    assert {v[1] for v in pc.HAUSDORFF.values()} == {0, 1, 5, 25} and {v[1] for v in pc.PLUS.values()} == {1, 5, 25}
    for cases in (pc.HAUSDORFF, pc.PLUS):
        assert {v[2] for v in cases.values()} == {2, 100, 256, 257, 1000, 1024}
    assert {v[3] for v in pc.HAUSDORFF.values()} | set(pc.RAGGED) == {None, 1, 1023, 1024, 1025, 4096, sum(pc.RAGGED)}
    lf = list(pc.LENSFIT.values())
    assert (pc.ROWS, pc.GROUPS) == (5, 2) and {v[1] for v in lf} == {0, 1, 5, 25}
    per = lambda n: -(-n // 256)                                                   # noqa: E731  points a thread holds
    assert {per(v[2]) for v in lf} == {1, 2, 3, 4} == {per(v[3]) for v in lf}
    assert {(2, 1), (100, 130), (257, 1023), (1024, 1024)} <= {(v[2], v[3]) for v in lf}
    assert {v[4] for v in lf} == {1, 2, 16} and {v[5] for v in lf} == {0, 1, 5} and {v[6] for v in lf} == {1.0, 0.25}
    assert all(("trace" in v[8]) == (v[5] > 0) for v in lf if len(v[8]) > 2)       # n_steps 0 has no trace
    full = [v for v in lf if set(v[8]) >= set(pc.LENSFIT_ALL[:-1])]
    assert len(full) >= len(lf) - 1 and any(v[8] == pc.LENSFIT_ALL for v in lf) and ("params", "loss") in {v[8] for v in lf}
    for name in pc.LENSFIT:                                                        # a NaN would pin nothing about the arithmetic
        assert all(np.isfinite(GOLD[k]).all() for k in GOLD.files if k.startswith(f"{name}/out/"))


def test_the_plus_fit_fixture_holds_every_case_and_is_small():
    assert {k.split("/")[0] for k in PF_GOLD.files} == set(pc.PLUSFIT) | {"build"} and "build/plusfit" in PF_GOLD.files
    assert os.path.getsize(PF_PATH) < 64 << 10
    pf = list(pc.PLUSFIT.values())
    per = lambda n: -(-n // 256)                                                   # noqa: E731  points a thread holds
    assert {v[1] for v in pf} == {0, 1, 5, 25} and {per(v[2]) for v in pf} == {1, 2, 3, 4} and {v[2] for v in pf} >= {2, 1024}
    assert {v[3] for v in pf} == {1, 2, 3, 16} and {v[4] for v in pf} == {0, 1, 5} and {v[5] for v in pf} == {1.0, 0.37}
    assert {v[6] for v in pf} == {False, True} and {v[7] for v in pf} == {0.0, 0.1}
    assert all(("trace" in v[8]) == (v[4] > 0) for v in pf if len(v[8]) > 2)       # n_steps 0 has no trace
    full = [v for v in pf if set(v[8]) >= set(pc.PLUSFIT_ALL[:-1])]
    assert len(full) == len(pf) - 1 and any(v[8] == pc.PLUSFIT_ALL for v in pf) and ("params", "loss") in {v[8] for v in pf}
    rows = pc.PLUSFIT_ROWS["pf_k5_p100_s2_n5_decay"]                               # the keep mask and the clamps under a step
    assert rows["zero_width"] and rows["clamped"] and pc.PLUSFIT["pf_k5_p100_s2_n5_decay"][4:7] == (5, 1.0, True)
    for name, case in pc.PLUSFIT.items():
        gold = {k.split("/")[2]: PF_GOLD[k] for k in PF_GOLD.files if k.startswith(f"{name}/out/")}
        if "n_run" not in gold:                                                    # (no early stop there: every start ran)
            assert case[7] == 0 and all(np.isfinite(v).all() for v in gold.values())
            continue
        n_run, S = gold["n_run"], case[3]
        assert sorted(set(n_run)) == ([1, 2, 3] if case[7] > 0 else [S])
        assert ((gold["best"] >= 0) & (gold["best"] < n_run)).all()
        ran = np.arange(S)[None, :] < n_run[:, None]
        # a start that ran holds finite words alone (a NaN would pin nothing about the arithmetic); one that did not holds what
        # the contract says: itself, +inf, and the quiet NaN 0x7fc00000 in grad and trace
        for k in ("params", "loss", "all_params", "all_loss", "grad", "trace"):
            if k in gold:
                assert np.isfinite(gold[k][ran] if k.startswith("all_") or k in ("grad", "trace") else gold[k]).all(), (name, k)
        assert np.array_equal(gold["all_params"][~ran], pc.inputs(name)["starts"][~ran])
        assert (gold["all_loss"][~ran] == np.inf).all() and (gold["grad"][~ran].view(np.uint32) == QNAN).all()
        if "trace" in gold:
            assert (gold["trace"][~ran].view(np.uint32) == QNAN).all()


@pytest.mark.parametrize("name", NAMES + list(pc.PLUSFIT))
def test_output_bits_are_the_recorded_ones(name):
    gold = PF_GOLD if name in pc.PLUSFIT else GOLD
    inp = pc.inputs(name)
    for k, v in inp.items():
        want = gold[f"{name}/in/{k}"]
        same = v == want if k == "max_dist" else pc.sha(v) == str(want)
        assert same, f"{name}: the generated input {k} drifted: look at the oracles' generators, not at the kernels"
    out = pc.run(name, inp)
    assert {f"{name}/out/{k}" for k in out} == {k for k in gold.files if k.startswith(f"{name}/out/")}
    for k, v in out.items():
        want = gold[f"{name}/out/{k}"]
        if k in pc.HASHED:
            assert pc.sha(v) == str(want), (name, k)
        else:
            assert v.dtype == want.dtype and v.shape == want.shape and v.dtype.itemsize == 4, (name, k)
            diff = np.nonzero(v.view(np.int32) != want.view(np.int32))
            assert len(diff[0]) == 0, (name, k, diff, v[diff], want[diff])
