"""The call-form ledger without a GPU (tests/call_forms.py): every family dispatches as declared at 256 and at 128 CUs, every
(form, family) pair the forms' source files call for has a case in tests/test_gpu_call_forms.py or a reason in the ledger, and -
with the float64 oracle alone, on the ledger's own rows - the natural mistake of every form moves a compared tensor by at least ten
times what the GPU test allows it."""
import functools
import os

import pytest
import torch

from hint_amd import _lib
import call_forms as cf
from instance_cases import CASES, compiled_instances
from wgrad_geometry import Dispatcher

CUS = (256, 128)
FACTOR = 10.0
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hint_amd", "csrc")


@pytest.mark.parametrize("cu", CUS)
def test_families_dispatch_as_declared(cu, capsys):
    lib = _lib.load()
    lines = []
    for fam in cf.FAMILIES:
        B = cf.resolve_B(lib, fam, cu)
        disp = Dispatcher(lib, fam.tree)
        for entry, n_chain in (("block", 1), ("chain", cf.N_BLOCKS)):
            d = disp(B, cu, n_chain)
            m = cf.family_mismatch(fam, d, B, entry)
            assert m is None, m
        d = disp(B, cu)
        lines.append(f"{fam.name:9s} B={B:5d} tiles={d['tiles']:4d} nw={d['nw']} nr={d['nr']} alt4={d['alt4']} grid={d['grid']:4d} "
                     f"dw_splits={d['dw_splits']:3d} dw_rows={d['dw_rows']:4d}  " + ", ".join(fam.expect[i] for i in (0, 2, 3)))
        if fam.batch != 37:         # the smallest ragged B that shows the field: one tile fewer does not
            field, value = fam.batch
            assert B % 16 == 1 and disp(B - 16, cu)[field] != value and disp(B - 1, cu)[field] != value, (fam.name, B)
        else:
            assert d["tiles"] == 3      # three tiles, the last one ragged
    with capsys.disabled():
        print(f"\ncall-form ledger at {cu} CUs:\n" + "\n".join(lines))


def test_families_are_the_instance_ledgers_trees():
    names = {c.name for c in CASES}
    for fam in cf.FAMILIES:
        assert fam.case in names, fam
    # the wave-local kernels as a single block and chained, row pairs, the three builds of hint_bwd.hip, both general forwards,
    # three of part B's four instances on the general side
    lib_path = _lib.LIB_PATH
    have = set(compiled_instances(lib_path))
    want = {s for fam in cf.FAMILIES for entry in ("block", "chain") for s in fam.expect_for(entry)}
    assert want <= have, sorted(want - have)
    assert {f.expect[2] for f in cf.FAMILIES} >= {"hint_wl_bwd_kernel<1, false>", "hint_wl_bwd_kernel<2, false>", "hint_bwd_kernel",
                                                   "hint_bwd_kernel_n3", "hint_bwd_kernel_fly"}
    assert {f.expect[0] for f in cf.FAMILIES} >= {"hint_apply_kernel<false, false>", "hint_apply_kernel<false, true>"}
    assert {f.expect[3] for f in cf.FAMILIES} == {"hint_wgrad_kernel<false, false>", "hint_wgrad_kernel<true, true>",
                                                   "hint_wgrad_kernel<false, true>"}


def test_forms_name_source_files_that_exist():
    for form in cf.FORMS:
        for f in form.files:
            assert os.path.exists(os.path.join(CSRC, f)), (form.name, f)
    for fam in cf.FAMILIES:
        for f in fam.files:
            assert os.path.exists(os.path.join(CSRC, f)), (fam.name, f)
    # the call forms' code: where the ledger says it is
    text = {f: open(os.path.join(CSRC, f)).read() for f in cf.FWD_FILES + cf.BWD_FILES + cf.DW_FILES}
    for f in cf.BWD_FILES:
        assert "blk.g_add" in text[f] and "gJ_const" in text[f] and "gz_scale" in text[f], f
    for f in cf.FWD_FILES:
        assert "J_in" in text[f] and "loss_acc" in text[f], f
    assert "blk.x_in" in text["hint_wgrad.hip"] and "blk.c_in" in text["hint_wgrad.hip"]


def test_every_pair_has_a_case_or_a_reason():
    import test_gpu_call_forms as T
    required = cf.required_pairs()
    assert len(required) == len(cf.FORMS) * len(cf.FAMILIES)       # every form's files reach every family: wave-local or general
    run = set()
    for group, fam in T.CASES:
        for form in cf.GROUPS[group]:
            assert form in T.COMPARES, f"{form}: no comparison in tests/test_gpu_call_forms.py"
            run.add((form, fam))
    for pair in required:
        assert (pair in run) != (pair in cf.EXCLUDED), f"{pair}: neither compared with the oracle nor excluded with a reason (or both)"
    for pair, why in cf.EXCLUDED.items():
        assert pair in required and why
    assert sorted(f for g in cf.GROUPS.values() for f in g) == sorted(cf.FORM)


@functools.lru_cache(maxsize=None)
def _rows(form, fam_name):
    lib = _lib.load()
    fam = cf.FAMILY[fam_name]
    return cf.ROWS[form](fam, cf.resolve_B(lib, fam, 256))


def _worst(ref, wrong):
    from test_gpu_instances import TOL_FWD, TOL_GW, TOL_GX
    refs = ref if isinstance(ref, (list, tuple)) else [ref]
    wrongs = wrong if isinstance(wrong, (list, tuple)) else [wrong]
    worst, where = 0.0, None
    for i, (r, w) in enumerate(zip(refs, wrongs)):
        for k, v in cf.ratios(w, r, (TOL_FWD, TOL_GX, TOL_GW)).items():
            if v > worst:
                worst, where = v, (i, k)
    return worst, where


SENSITIVITY = [(fo.name, m, fa.name) for fo in cf.FORMS for m in fo.mistakes for fa in cf.FAMILIES
               if (fo.name, fa.name) in cf.pairs() and (m, fa.name) not in cf.MISTAKE_EXCLUDED]


def test_every_mistake_is_listed_or_excluded():
    want = {"g_add dropped on block 1", "g_add behind the permutation", "J_in dropped", "gz_scale taken as 1", "gJ_const ignored",
            "c_in replaced by another block's c", "x_in replaced by the first block's x", "top slice replaced by the unpermuted x"}
    assert want <= {m for fo in cf.FORMS for m in fo.mistakes}
    for fa in cf.FAMILIES:
        for fo in cf.FORMS:
            for m in fo.mistakes:
                assert ((fo.name, m, fa.name) in SENSITIVITY) != ((m, fa.name) in cf.MISTAKE_EXCLUDED)
    assert {fa for _, fa in cf.MISTAKE_EXCLUDED} == {f.name for f in cf.FAMILIES if f.dc == 0}


@pytest.mark.parametrize("fam_name", [f.name for f in cf.FAMILIES])
def test_a_natural_mistake_is_far_over_the_bound(fam_name):
    """what the GPU comparison rests on: on the ledger's own rows (256 CUs) every natural mistake of every form moves at least one
    compared tensor by FACTOR times its bound or more, and the right oracle passes its own comparison"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    fam = cf.FAMILY[fam_name]
    refs = {}
    low = []
    for form, mistake, fa in SENSITIVITY:
        if fa != fam_name:
            continue
        rows = _rows(form, fam_name)
        if form not in refs:
            refs[form] = cf.ORACLES[form](fam, rows)
            assert _worst(refs[form], refs[form])[0] == 0.0
        wrong = cf.ORACLES[form](fam, rows, mistake)
        worst, where = _worst(refs[form], wrong)
        print(f"{fam_name} {form} '{mistake}': {worst:.3g} times the bound at {where}")
        if not worst >= FACTOR:
            low.append((form, mistake, worst, where))
    assert not low, low
