"""hint_hausdorff_run and hint_plus_run give, on the cases of tests/pointset_cases.py, the bits that tests/golden/pointset_bits.npz
recorded before the two kernels were built from one shared core (hint_amd/csrc/hint_pointset.hpp): every output compared as
int32 words, exactly.  A generator that drifted is told apart from a kernel that did: the fixture holds a sha256 of every input."""
import os

import numpy as np
import pytest

import pointset_cases as pc

pytestmark = pytest.mark.gpu

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointset_bits.npz")
GOLD = np.load(PATH)


def test_the_fixture_holds_every_case_and_is_small():
    names = list(pc.HAUSDORFF) + list(pc.PLUS)
    assert {k.split("/")[0] for k in GOLD.files} == set(names) | {"build"}
    assert os.path.getsize(PATH) < 64 << 10
    assert {v[1] for v in pc.HAUSDORFF.values()} == {0, 1, 5, 25} and {v[1] for v in pc.PLUS.values()} == {1, 5, 25}
    for cases in (pc.HAUSDORFF, pc.PLUS):
        assert {v[2] for v in cases.values()} == {2, 100, 256, 257, 1000, 1024}
    assert {v[3] for v in pc.HAUSDORFF.values()} | set(pc.RAGGED) == {None, 1, 1023, 1024, 1025, 4096, sum(pc.RAGGED)}


@pytest.mark.parametrize("name", list(pc.HAUSDORFF) + list(pc.PLUS))
def test_output_bits_are_the_recorded_ones(name):
    inp = pc.inputs(name)
    for k, v in inp.items():
        want = GOLD[f"{name}/in/{k}"]
        same = v == want if k == "max_dist" else pc.sha(v) == str(want)
        assert same, f"{name}: the generated input {k} drifted: look at the oracles' generators, not at the kernels"
    out = pc.run(name, inp)
    assert {f"{name}/out/{k}" for k in out} == {k for k in GOLD.files if k.startswith(f"{name}/out/")}
    for k, v in out.items():
        want = GOLD[f"{name}/out/{k}"]
        if k in pc.HASHED:
            assert pc.sha(v) == str(want), (name, k)
        else:
            assert v.dtype == want.dtype and v.shape == want.shape and v.dtype.itemsize == 4, (name, k)
            diff = np.nonzero(v.view(np.int32) != want.view(np.int32))
            assert len(diff[0]) == 0, (name, k, diff, v[diff], want[diff])
