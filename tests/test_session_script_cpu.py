"""CPU calibration of the trainer sessions (tests/session_script.py): the tolerances the GPU session test uses are 4 x the
float32 oracle's own deviation from the float64 oracle, and every injected fault - the silent failures a trainer's state between
calls can have - moves at least one compared quantity by 5 x its tolerance.  A script that cannot satisfy both is shortened or
reordered; the tolerance is not widened.  Also: the trainers' input validator (hint._as_input) on the refusals that need no GPU."""
import numpy as np
import pytest
import torch

import session_script as ss


@pytest.mark.parametrize("flow_name", list(ss.FLOWS))
@pytest.mark.parametrize("script", list(ss.SCRIPTS))
def test_float32_floor_and_injected_faults(script, flow_name):
    ref = ss.reference(script, flow_name)
    floors = ss.floors(script, flow_name)
    tol = ss.tolerances(script, flow_name)
    print(f"\n{script}/{flow_name}: floors " + " ".join(f"{k}={v:.1e}" for k, v in floors.items())
          + " | tolerances " + " ".join(f"{k}={v:.1e}" for k, v in tol.items()))
    print(f"    training rows left out next to a ReLU kink: {ref['dropped']} of {ref['picked']}")
    assert 0 <= ref["dropped"] <= ss.MAX_DROPPED * ref["picked"], (ref["dropped"], ref["picked"])
    assert len(ref["losses"]) >= 6 and np.all(np.isfinite(ref["losses"]))
    assert np.abs(ref["losses"]).max() < 1e3              # (a flow that expands its input would put float32 itself out of reach)
    for k in tol:
        # the float32 oracle passes the tolerance it sets with room to spare, and the tolerance is no looser than the existing test's
        assert floors[k] <= tol[k] / 4.0 + 1e-30 or tol[k] == ss.CAPS[k], (k, floors[k], tol[k])
        assert floors[k] < ss.CAPS[k] / 4.0, (k, floors[k])
        assert 4.0 * ss.ULP <= tol[k] <= ss.CAPS[k], (k, tol[k])
    for fault in ss.FAULTS:
        dev = ss.deviations(ss.run_oracle(script, flow_name, fault=fault), ref)
        ratio = {k: dev[k] / tol[k] for k in tol}
        worst = max(ratio, key=ratio.get)
        print(f"    {fault:15s} moves {worst} by {ratio[worst]:.1e} x its tolerance")
        assert ratio[worst] >= 5.0, (fault, ratio)


@pytest.mark.parametrize("script,flow_name", list(ss.NOISY_SESSIONS), ids=["-".join(k) for k in ss.NOISY_SESSIONS])
def test_noisy_float32_floor_and_injected_noise_faults(script, flow_name):
    """the sessions with the training noise on (x + noise * the noise oracle's draws of the step): calibrated as the noise-free
    ones, and each injected noise fault - draws one step behind from the first shape change on, the gradient taken at x instead
    of x_noisy, every 16-row tile with tile 0's draws - moves a compared quantity by 5 tolerances at the session's level"""
    noise = ss.NOISY_SESSIONS[(script, flow_name)]
    assert noise in ss.NOISE_LEVELS
    assert ss.noise_level(script, flow_name) == noise      # the first level at which every fault is seen (0.01: the default)
    ref = ss.reference(script, flow_name, noise)
    floors = ss.floors(script, flow_name, noise)
    tol = ss.tolerances(script, flow_name, noise)
    print(f"\n{script}/{flow_name} noise={noise}: floors " + " ".join(f"{k}={v:.1e}" for k, v in floors.items())
          + " | tolerances " + " ".join(f"{k}={v:.1e}" for k, v in tol.items()))
    print(f"    training rows replaced next to a ReLU kink: {ref['dropped']} of {ref['picked']}")
    assert 0 <= ref["dropped"] <= ss.MAX_DROPPED * ref["picked"], (ref["dropped"], ref["picked"])
    assert len(ref["losses"]) >= 6 and np.all(np.isfinite(ref["losses"]))
    assert np.abs(ref["losses"]).max() < 1e3
    # the noise is on: the session is not the noise-free one
    assert ss.scalar_dev(ref["losses"], ss.reference(script, flow_name)["losses"]) > 100 * tol["losses"]
    for k in tol:
        assert floors[k] <= tol[k] / 4.0 + 1e-30 or tol[k] == ss.CAPS[k], (k, floors[k], tol[k])
        assert floors[k] < ss.CAPS[k] / 4.0, (k, floors[k])
        assert 4.0 * ss.ULP <= tol[k] <= ss.CAPS[k], (k, tol[k])
    ratios = ss.fault_ratios(script, flow_name, noise)
    assert set(ratios) == set(ss.NOISE_FAULTS)
    for fault, (worst, ratio) in ratios.items():
        print(f"    {fault:22s} moves {worst} by {ratio:.1e} x its tolerance")
        assert ratio >= ss.DETECT == 5.0, (fault, worst, ratio)


def test_noisy_rows_are_judged_as_the_step_sees_them():
    """pick_rows with noise on: the chosen rows, perturbed by POSITION with the draws of the step to come, keep KINK away from every
    ReLU kink; a position is re-filled from the unused candidates; without noise the rule is the old one"""
    spec = ss.FLOWS["wl_d6"]
    be = ss.OracleBackend(spec, noise=0.25)
    x, c = ss.draw("epochs", 0, spec, (ss.FULL,), ss.SPARE)
    kink, ss.KINK = ss.KINK, 2e-6                # (a wider band, so that some rows do fall into it: as drawn, and when perturbed)
    try:
        idx = be.pick_rows(x, c, ss.FULL)
        assert len(set(idx.tolist())) == ss.FULL
        xn = be.perturbed(x[idx].double(), 1)
        assert torch.equal(xn, x[idx].double() + 0.25 * be.draws(1, ss.FULL, spec["d"]))
        assert float(be.kink_distance(xn, None).min()) > ss.KINK
        assert be.dropped > 0 and be.picked == ss.FULL
        plain = ss.OracleBackend(spec)
        first = torch.nonzero(plain.kink_distance(x, c) > ss.KINK).flatten()[:ss.FULL]
        assert torch.equal(plain.pick_rows(x, c, ss.FULL), first)
    finally:
        ss.KINK = kink
    # the draws of a step: position-keyed, the oracle's stream, float32 for the float32 backend
    import noise_oracle as no
    N = be.draws(3, 40, spec["d"])
    assert N.dtype == torch.float64 and np.array_equal(N.numpy().reshape(-1), no.normals(ss.NOISE_SEED, 3, 40 * spec["d"]))
    T = be.draws(3, 40, spec["d"], tile_repeat=True)
    assert torch.equal(T[:16], N[:16]) and torch.equal(T[16:32], N[:16]) and torch.equal(T[32:], N[:8])
    assert ss.OracleBackend(spec, torch.float32, noise=0.25).draws(3, 40, spec["d"]).dtype == torch.float32


def test_scripts_hold_what_the_sessions_are_about():
    ep = ss.SCRIPTS["epochs"]
    steps = [e for e in ep if e[0] == "step"]
    assert steps[2][1] != steps[0][1]                     # the first shape change within the first five steps
    assert {e[0] for e in ep} >= {"step", "eval_nll", "sample", "set_lr"}
    ms = ss.SCRIPTS["many_sizes"]
    first = ms[0]
    assert first[0] == "step_many"
    sizes = {e[1] for e in ms if e[0] == "step"} - {first[2]}
    assert len(sizes) >= 10 and 1 in sizes
    assert ("step_many",) + first[1:] in ms[1:]           # the return to the first size, on the same graph shape
    mx = [e[0] for e in ss.SCRIPTS["mixed"]]
    assert mx[:2] == ["step_many", "step"] and "input_buffers" in mx and "repack" in mx
    assert mx[mx.index("input_buffers") - 1] == "step_many"      # a capture by input_buffers() right behind a step_many()
    for flow in ss.FLOWS.values():
        for script, events in ss.SCRIPTS.items():
            for i, ev in enumerate(events):
                if ev[0] in ("step", "eval_nll", "sample"):
                    a, _ = ss.draw(script, i, flow, (ev[1],), ss.SPARE)
                    b, _ = ss.draw(script, i, flow, (ev[1],), ss.SPARE)
                    assert torch.equal(a, b) and a.dtype == torch.float32 and b.shape[0] == ev[1] + ss.SPARE


# ---- the validator, where no GPU is needed (the device is whatever the caller's model is on) --------------------------------
def test_as_input_contract_on_the_cpu():
    from hint_amd.hint import HintAmdError, _as_input
    cpu = torch.device("cpu")
    x = torch.randn(7, 6)
    assert _as_input(x, "x", cpu, 6) is x                 # contiguous fp32: the tensor itself (a graph's input buffer stays one)
    wide = torch.randn(7, 9)
    for t in (torch.randn(6, 7).t(), wide[:, 2:8], x.double(), x.half(), x.bfloat16(), wide.double()[:, 1:7]):
        got = _as_input(t, "x", cpu, 6)
        assert got.dtype == torch.float32 and got.is_contiguous() and got.stride() == (6, 1)
        assert torch.equal(got, t.float().contiguous())
    xs = torch.randn(5, 3, 6).transpose(0, 1)             # [K, B, d] made from a [B, K, d] table
    got = _as_input(xs, "xs", cpu, 6, rank=3)
    assert got.is_contiguous() and torch.equal(got, xs.contiguous())
    for bad in (torch.zeros(7, 6, dtype=torch.int64), torch.zeros(7, 6, dtype=torch.bool), torch.zeros(7, 6, dtype=torch.int32)):
        with pytest.raises(HintAmdError, match="dtype"):
            _as_input(bad, "x", cpu, 6)
    with pytest.raises(HintAmdError, match="is on"):
        _as_input(torch.empty(7, 6, device="meta"), "x", cpu, 6)
    with pytest.raises(HintAmdError, match="is on"):      # a host batch for a model on a GPU: refused, never handed to a kernel
        _as_input(x, "x", torch.device("cuda", 0), 6)
    for bad in (torch.randn(6), torch.randn(7, 5), torch.randn(2, 7, 6), torch.randn(6, 7)):
        with pytest.raises(HintAmdError, match="must be"):
            _as_input(bad, "x", cpu, 6)
    with pytest.raises(HintAmdError, match="must be"):
        _as_input(x, "xs", cpu, 6, rank=3)
    with pytest.raises(HintAmdError, match="leading shape"):
        _as_input(torch.randn(8, 2), "c", cpu, 2, rows=(7,))
    with pytest.raises(HintAmdError, match="tensor"):
        _as_input(x.numpy(), "x", cpu, 6)
