"""Trainer SESSIONS: scripted sequences of the calls a real training run makes on one live trainer - steps at changing batch
shapes, step_many, evaluation, sampling, a module forward, learning-rate decay, input_buffers, repack - and a runner that applies
such a script to an `OracleFlow` in float64 (clamp + Adam as OracleFlow.train_step, the reference loop).  TEST INFRASTRUCTURE.

tests/test_session_script_cpu.py calibrates the scripts on the CPU; tests/test_gpu_trainer_session.py runs them on FlowTrainer.

Tolerances are MEASURED, not chosen: for every (script, flow) `tolerances()` runs the float32 oracle against the float64 oracle
and takes 4 x that deviation (the GPU sums in another fp32 order of the same class), never more than what
test_trainer_reproduces_reference_adam_steps grants (CAPS) and never less than 4 x one fp32 ulp (2^-23: no fp32 result can be
asked to be closer than its own format).  The deviations:
    losses / nll   max over the events of |a - b| / (0.1 + |b|)   (rtol 1e-4, atol 1e-5 of the existing test = 1e-4 of that scale)
    update         per parameter tensor |(final - initial) - (final_ref - initial)| / |final_ref - initial| (check_update of
                   test_gpu_flow.py), the worst tensor

Measured on the CPU (float32 oracle vs float64 oracle; `pytest tests/test_session_script_cpu.py -s` prints them):
    floor     script        wl_d6   gen_d43   cond_d9  unchained_d8
    losses    epochs         2.7e-06   9.2e-08   7.9e-08   3.4e-07
              many_sizes     2.1e-07   2.1e-07   2.2e-07   5.3e-07
              mixed          1.6e-07   1.4e-07   1.7e-07   5.0e-07
    nll       epochs         2.7e-08   4.4e-08   3.9e-08   6.7e-08
              many_sizes     2.9e-08   1.3e-08   2.1e-09   1.4e-08
              mixed          3.3e-08   8.2e-09   2.3e-08   2.1e-08
    update    epochs         1.4e-04   4.7e-05   2.0e-03   5.0e-05
              many_sizes     3.6e-05   1.0e-04   8.7e-05   1.4e-04
              mixed          1.2e-05   2.6e-05   2.7e-05   2.0e-05
  (every nll floor lies under one fp32 ulp, 1.2e-07: the nll tolerance is 4 ulp = 4.8e-07 everywhere.  The figures move with the
   CPU's thread count - the float32 sums change order - so the tests compute them where they run instead of reading them here.
   Between 0 and 17 candidate rows per session are left out next to a ReLU kink.)
Injected faults (float64 oracle with the fault against the one without): the quantity each one moves most, as a multiple of its
tolerance; the smallest such multiple over the four flows:
    fault             epochs           many_sizes       mixed
    bias_ahead        losses 1.3e+03   losses 2.4e+03   losses 3.2e+03
    lr_dropped        nll    6.3e+03   losses 4.1e+04   losses 6.4e+04
    ragged_skipped    losses 9.6e+03   losses 1.3e+04   losses 2.0e+04
    stale_weights     losses 2.0e+04   losses 2.7e+04   losses 2.1e+04
    prev_loss         losses 1.8e+04   losses 2.6e+05   losses 4.7e+04

NOISY SESSIONS (NOISY_SESSIONS: `epochs` on every flow, `mixed` on wl_d6 and gen_d43): the t-th training step trains on
x + noise * normals(NOISE_SEED, t, B * d) of tests/noise_oracle.py, calibrated the same way (float32 oracle on the same draws
against the float64 oracle, x 4, floor 4 ulp, the same caps).  Floors measured on the CPU at noise = 0.01:
    floor     script   wl_d6     gen_d43   cond_d9   unchained_d8
    losses    epochs   1.2e-07   9.4e-08   1.3e-07   4.3e-07
              mixed    1.1e-07   1.8e-07
    nll       epochs   1.9e-08   4.4e-08   9.6e-08   4.6e-08
              mixed    3.3e-09   4.8e-10
    update    epochs   3.7e-05   6.8e-05   8.5e-04   4.6e-05
              mixed    1.2e-05   2.3e-05
  (0 to 9 candidate rows per session give their position to a spare next to a ReLU kink.)
Injected noise faults, each against the fault-free float64 run AT THE TRAINERS' DEFAULT noise = 0.01 - every one is seen there in
every flow, so no session needed the higher levels 0.1 / 0.25 (noise_level() would find them): the quantity moved most, as a
multiple of its tolerance
    fault                   script   wl_d6            gen_d43          cond_d9          unchained_d8
    noise_step_behind       epochs   losses 1.8e+04   losses 1.6e+03   losses 4.5e+03   losses 7.7e+02
                            mixed    losses 5.7e+03   update 1.2e+03
    noise_not_in_backward   epochs   losses 1.7e+04   update 1.2e+03   update 2.8e+02   update 1.2e+03
                            mixed    losses 5.0e+03   update 2.8e+03
    noise_tile_repeat       epochs   losses 4.2e+04   update 2.3e+03   losses 6.8e+03   update 1.6e+03
                            mixed    losses 1.5e+04   update 2.7e+03
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import noise_oracle as no
from oracle import hint_oracle as orc

# ---- flows ------------------------------------------------------------------------------------------------------------------
FLOWS = {
    "wl_d6":        dict(d=6, widths=(140, 70, 35, 17), n_blocks=3, dc=0, use_chain=True),     # wave-local kernels
    "gen_d43":      dict(d=43, widths=(67, 33, 16, 8), n_blocks=2, dc=0, use_chain=True),      # general kernels, subtree groups
    "cond_d9":      dict(d=9, widths=(19, 11, 3), n_blocks=4, dc=2, use_chain=True),           # conditional
    "unchained_d8": dict(d=8, widths=(24, 12), n_blocks=2, dc=0, use_chain=False),             # block-by-block launches
}

# ---- scripts ----------------------------------------------------------------------------------------------------------------
# events: ("step", B) ("step_many", K, B) ("eval_nll", B) ("sample", B) ("module_forward", B) ("set_lr", factor)
#         ("input_buffers", B): a step whose batch is written into the trainer's own input buffer
#         ("repack",): every parameter scaled in place by REPACK_SCALE from outside the trainer, then trainer.repack()
REPACK_SCALE = 1.0 - 2.0 ** -7
FULL, RAGGED, EVAL = 256, 173, 300


def _epoch():
    return [("step", FULL), ("step", FULL), ("step", RAGGED), ("eval_nll", EVAL), ("eval_nll", EVAL), ("eval_nll", 41),
            ("sample", 64), ("module_forward", 96), ("set_lr", 0.5)]


SCRIPTS = {
    # two epochs: full batches, a ragged last batch (the first shape change is step 3: the bias correction still moves by 12 %
    # per step there), an evaluation loop at a third size with its own ragged end, sample(), lr *= 0.5
    "epochs": _epoch() + _epoch(),
    # a step_many graph captured at the first size stays live while step() walks through eleven other sizes (a chain per size:
    # more than the eight the trainer keeps), then the first size again on the live graph
    "many_sizes": [("step_many", 2, FULL)] + [("step", b) for b in (1, 5, 9, 33, 64, 100)] + [("set_lr", 0.5)]
    + [("step", b) for b in (RAGGED, 200, 255, 300, 411)] + [("eval_nll", EVAL), ("step_many", 2, FULL), ("step", FULL),
                                                               ("sample", 64)],
    # step_many, step at another size, step_many at the first size again (the live graph), input_buffers at a size never seen
    # (its capture comes right behind a step_many), weights changed from outside, step_many at another K (re-capture)
    "mixed": [("step_many", 3, FULL), ("step", RAGGED), ("set_lr", 0.5), ("step_many", 3, FULL), ("input_buffers", EVAL),
              ("repack",), ("step", RAGGED), ("eval_nll", EVAL), ("module_forward", 96), ("step_many", 2, FULL), ("sample", 64),
              ("input_buffers", FULL), ("step", FULL)],
}

FAULTS = ("bias_ahead", "lr_dropped", "ragged_skipped", "stale_weights", "prev_loss")
# ---- sessions with the training noise on --------------------------------------------------------------------------------------
# The t-th training step of a session (t = 1, 2, ...: the trainers' step prologue advances the device counter BEFORE the forward)
# trains on x + noise * normals(NOISE_SEED, t, B * d) (tests/noise_oracle.py), the draw of flat element f on element f of the batch.
NOISE_FAULTS = ("noise_step_behind", "noise_not_in_backward", "noise_tile_repeat")
NOISE_SEED = 1234
NOISE_LEVELS = (0.01, 0.1, 0.25)                                      # the trainers' default first; see noise_level()
# the noisy sessions and the level each runs at: what noise_level() finds (tests/test_session_script_cpu.py asserts the table, so
# that the GPU tests need not run the fault calibration) - every fault shows at the trainers' default in every one of them
NOISY_SESSIONS = {("epochs", "wl_d6"): 0.01, ("epochs", "gen_d43"): 0.01, ("epochs", "cond_d9"): 0.01,
                  ("epochs", "unchained_d8"): 0.01, ("mixed", "wl_d6"): 0.01, ("mixed", "gen_d43"): 0.01}
TILE_ROWS = 16                                                        # the row kernels' tile (noise_tile_repeat)

LR, BETAS, EPS, WD = 0.01 * 3e-2, (0.9, 0.95), 1e-4, 1.86e-5          # FlowTrainer's defaults (train_unconditional.py:174-176)
CAPS = dict(losses=1e-4, nll=1e-4, update=5e-2)                       # test_trainer_reproduces_reference_adam_steps
ULP = 2.0 ** -23
INIT_SCALE = 0.5
TOL_FWD = 1e-5                                                        # sample() x and J


KINK = 5e-7          # as tests/test_gpu_chain_workloads.py: a hidden pre-activation this close to zero (of its layer's largest in that row)
SPARE = 24           # candidate rows drawn beyond a training batch's size
# The most training rows a session may leave out, as a share of the rows it trains on - so that the rule cannot grow into a filter
# that decides the comparison.  A hidden unit's pre-activation lies within KINK of zero (of its row's largest, some 3 sigma) with
# a probability of about 2 * KINK * 3 * 0.4 = 1.2e-6; the largest flow here has some 7e3 hidden units per row (3 blocks x 7 nodes
# x 2 subnets x 2 hidden layers, 140 .. 35 wide): under 1 % of its rows, less for the others.
MAX_DROPPED = 0.01


def draw(script: str, index: int, spec, rows, spare: int = 0):
    """the rows of event `index`: float32 values (both the trainer and the float64 oracle see exactly these), from a generator
    seeded by the event - a fault that skips an event shifts no later batch.  spare: that many candidate rows more"""
    g = torch.Generator().manual_seed(7919 * (1 + sorted(SCRIPTS).index(script)) + index)
    rows = tuple(rows[:-1]) + (rows[-1] + spare,)
    x = torch.randn(*rows, spec["d"], generator=g, dtype=torch.float32)
    c = torch.randn(*rows, spec["dc"], generator=g, dtype=torch.float32) if spec["dc"] > 0 else None
    return x, c


def _take(t, idx):
    return t[idx] if t is not None else None


def initial_weights(spec):
    """-> (per-block parameter dicts, perms) in float32: the start of the trainer and, cast up, of the oracle.  torch's default
    Linear init at INIT_SCALE: at full scale the d = 43 and the conditional flow expand their input to losses of 1e6..1e9, where
    float32 itself is 1e-4 off the float64 oracle; at half scale s and t are still far from zero (-log|det J| of 2.5 .. -5)"""
    dims_c = [(spec["dc"],)] if spec["dc"] > 0 else ()
    flow = orc.OracleFlow(spec["d"], spec["n_blocks"], list(spec["widths"]), dims_c=dims_c, seed=11, init_scale=None,
                          dtype=torch.float32)
    return [{k: v * INIT_SCALE for k, v in P.items()} for P in flow.params], flow.perms


def run_session(script: str, spec, backend, rows=None):
    """apply the script's events to a backend (OracleBackend here, the trainer's in test_gpu_trainer_session.py) -> the record:
    losses [n_steps, 2], nll [n_eval], samples [(x, J)], forwards [(z, J)], rows.
    Training batches are the first B of B + SPARE candidate rows that keep every hidden pre-activation KINK away from zero in the
    float64 oracle AT ITS WEIGHTS OF THAT STEP (rows=None: this backend decides - the reference run; otherwise its record's
    `rows`): next to a ReLU kink float32 summation order decides the side, either subgradient is a correct answer, and one
    flipped unit moves that node's update by 1e-3 (measured: NOTES.md) - the forward of such rows is not ambiguous, so evaluation,
    sampling and module-forward batches are taken as drawn."""
    rec = dict(losses=[], nll=[], samples=[], forwards=[], rows={})
    for i, ev in enumerate(SCRIPTS[script]):
        kind = ev[0]
        if kind in ("step", "input_buffers"):
            x, c = draw(script, i, spec, (ev[1],), SPARE)
            idx = backend.pick_rows(x, c, ev[1]) if rows is None else rows[i]
            rec["rows"][i] = idx
            rec["losses"].append(list(getattr(backend, kind)(x[idx], _take(c, idx))))
        elif kind == "step_many":
            xs, cs = draw(script, i, spec, (ev[1], ev[2]), SPARE)
            if rows is None:            # (the weights move between the iterations: one at a time)
                rec["rows"][i] = []
                for k in range(ev[1]):
                    idx = backend.pick_rows(xs[k], _take(cs, k), ev[2])
                    rec["rows"][i].append(idx)
                    rec["losses"].append(list(backend.step(xs[k][idx], _take(cs, k)[idx] if cs is not None else None)))
            else:
                rec["rows"][i] = rows[i]
                xk = torch.stack([xs[k][idx] for k, idx in enumerate(rows[i])])
                ck = torch.stack([cs[k][idx] for k, idx in enumerate(rows[i])]) if cs is not None else None
                rec["losses"] += [list(p) for p in backend.step_many(xk, ck)]
        elif kind == "eval_nll":
            rec["nll"].append(backend.eval_nll(*draw(script, i, spec, (ev[1],))))
        elif kind == "sample":
            rec["samples"].append(backend.sample(*draw(script, i, spec, (ev[1],))))
        elif kind == "module_forward":
            rec["forwards"].append(backend.module_forward(*draw(script, i, spec, (ev[1],))))
        elif kind == "set_lr":
            backend.set_lr(ev[1])
        elif kind == "repack":
            backend.repack(REPACK_SCALE)
        else:
            raise ValueError(ev)
        backend.after_event(i, ev)
    rec["losses"] = np.array(rec["losses"], dtype=np.float64).reshape(-1, 2)
    rec["nll"] = np.array(rec["nll"], dtype=np.float64)
    return rec


class OracleBackend:
    """the session on an OracleFlow in `dtype`; `fault` injects one of FAULTS (the calibration's sensitivity check)"""

    def __init__(self, spec, dtype=torch.float64, fault=None, noise=0.0, seed=NOISE_SEED):
        assert fault is None or fault in FAULTS or (fault in NOISE_FAULTS and noise > 0)
        self.noise, self.seed, self.t = float(noise), int(seed), 0     # t: training steps taken (the trainers' step counter)
        self.behind = False                                            # noise_step_behind has set in
        dims_c = [(spec["dc"],)] if spec["dc"] > 0 else ()
        self.flow = orc.OracleFlow(spec["d"], spec["n_blocks"], list(spec["widths"]), dims_c=dims_c, dtype=dtype)
        params, perms = initial_weights(spec)
        self.flow.params = [{k: v.to(dtype).clone() for k, v in P.items()} for P in params]
        self.flow.perms = [None if W is None else W.to(dtype) for W in perms]
        self.initial = [{k: v.clone() for k, v in P.items()} for P in self.flow.params]
        self.flow.make_optimizer(lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
        self.dtype, self.fault = dtype, fault
        self.first_B = self.last_B = None
        self.prev_pair = None
        self.prev_weights = None
        self.pending = {f: True for f in FAULTS}            # every fault fires once

    def _cast(self, x, c):
        return x.to(self.dtype), ([c.to(self.dtype)] if c is not None else ())

    def draws(self, t, B, d, tile_repeat=False):
        """[B, d] in the backend's dtype: the noise oracle's draws of step t, flat element f of the batch -> draw f"""
        np_dt = np.float64 if self.dtype == torch.float64 else np.float32
        N = torch.from_numpy(no.normals(self.seed, t, B * d, np_dt).reshape(B, d).copy())
        if tile_repeat:                                     # every 16-row tile the draws of tile 0
            N = N[torch.arange(B) % TILE_ROWS]
        return N

    def perturbed(self, xd, t, tile_repeat=False):
        """x + noise * N(seed, t), multiplied and added in the backend's dtype (as the kernels do in fp32)"""
        if self.noise == 0.0:
            return xd
        return xd + torch.tensor(self.noise, dtype=self.dtype) * self.draws(t, xd.shape[0], xd.shape[1], tile_repeat)

    @torch.no_grad()
    def kink_distance(self, x, c):
        """per row: the smallest hidden pre-activation's distance from zero, of its layer's largest in that row (whole chain,
        current weights)"""
        dist = torch.full((x.shape[0],), float("inf"), dtype=torch.float64)
        relu = torch.relu

        def spy(t):
            nonlocal dist
            if t.numel() > 0:
                a = t.detach().abs().reshape(t.shape[0], -1).double()
                dist = torch.minimum(dist, a.min(dim=1).values / a.max(dim=1).values.clamp(min=1e-3))
            return relu(t)
        torch.relu = spy
        try:
            xd, cd = self._cast(x, c)
            self.flow.forward(xd, cd)
        finally:
            torch.relu = relu
        return dist

    @torch.no_grad()
    def pick_rows(self, x, c, B):
        """the first B candidate rows none of whose hidden pre-activations (whole chain, current weights) lies within KINK of
        zero (rows_off_the_kinks of test_gpu_chain_workloads.py).
        With noise the kinks are judged on the rows AS THE STEP SEES THEM, and a draw belongs to a position in the batch, not to a
        candidate: the first B good candidates are perturbed by position with the draws of the step to come; a row that now lies
        within KINK gives its position to the next unused candidate; again until the batch is clean."""
        dist = self.kink_distance(x, c)
        idx = torch.nonzero(dist > KINK).flatten()[:B]
        assert idx.numel() == B, (idx.numel(), B)
        self.picked = getattr(self, "picked", 0) + B
        if self.noise == 0.0:
            self.dropped = getattr(self, "dropped", 0) + int(idx[-1]) + 1 - B
            return idx
        idx = idx.clone()
        used = set(idx.tolist())
        spare = [j for j in range(x.shape[0]) if j not in used]        # (candidates next to a kink as drawn may do when perturbed)
        dropped = 0
        while True:
            xn = self.perturbed(x[idx].to(self.dtype), self.t + 1)
            bad = torch.nonzero(self.kink_distance(xn, _take(c, idx)) <= KINK).flatten().tolist()
            if not bad:
                break
            for pos in bad:
                assert spare, "no spare candidate row left"
                idx[pos] = spare.pop(0)
                dropped += 1
        self.dropped = getattr(self, "dropped", 0) + dropped
        return idx

    def _fire(self, fault, when) -> bool:
        if self.fault == fault and self.pending[fault] and when:
            self.pending[fault] = False
            return True
        return False

    def step(self, x, c):
        B = x.shape[0]
        if self.first_B is None:
            self.first_B = B
        changed = self.last_B is not None and B != self.last_B
        self.last_B = B
        flow, opt = self.flow, self.flow.opt
        xd, cd = self._cast(x, c)
        self.t += 1
        x_clean = xd
        if self.noise > 0:
            self.behind = self.behind or (self.fault == "noise_step_behind" and changed)    # from the first shape change on
            xd = self.perturbed(xd, self.t - 1 if self.behind else self.t, tile_repeat=self.fault == "noise_tile_repeat")
        if self._fire("bias_ahead", changed):               # the device step counter one ahead from the first shape change on
            for st in opt.state.values():
                st["step"] += 1
        if self._fire("ragged_skipped", B != self.first_B):  # the first batch of another size: evaluated, not trained on
            with torch.no_grad():
                pair = [float(v) for v in flow.loss_terms(*flow.forward(xd, cd))]
            self.prev_pair = pair
            return pair
        before = [p.detach().clone() for p in flow.parameters()]
        if self._fire("stale_weights", changed and self.prev_weights is not None):
            # forward and backward on the weights of the step before (a stale packed copy); the update lands on the current ones
            now = [p.detach().clone() for p in flow.parameters()]
            with torch.no_grad():
                for p, w in zip(flow.parameters(), self.prev_weights):
                    p.copy_(w)
            opt.zero_grad()
            l0, l1 = flow.loss_terms(*flow.forward(xd, cd))
            (l0 + l1).backward()
            with torch.no_grad():
                for p, w in zip(flow.parameters(), now):
                    p.copy_(w)
            for p in flow.parameters():
                p.grad.data.clamp_(-5.0, 5.0)
            opt.step()
            pair = [float(l0), float(l1)]
        elif self.fault == "noise_not_in_backward":          # the loss at x_noisy, the gradient at x
            with torch.no_grad():
                pair = [float(v) for v in flow.loss_terms(*flow.forward(xd, cd))]
            opt.zero_grad()
            l0, l1 = flow.loss_terms(*flow.forward(x_clean, cd))
            (l0 + l1).backward()
            for p in flow.parameters():
                p.grad.data.clamp_(-5.0, 5.0)
            opt.step()
        else:
            pair = list(flow.train_step(xd, cd))
        self.prev_weights = before
        out = pair
        if self._fire("prev_loss", changed and self.prev_pair is not None):
            out = self.prev_pair                             # the loss read from the accumulator of the step before
        self.prev_pair = pair
        return out

    input_buffers = step

    def step_many(self, xs, cs):
        return [self.step(xs[k], cs[k] if cs is not None else None) for k in range(xs.shape[0])]

    @torch.no_grad()
    def eval_nll(self, x, c):
        return self.flow.nll(*self.flow.forward(*self._cast(x, c)))

    @torch.no_grad()
    def sample(self, z, c):
        x, J = self.flow.inverse(*self._cast(z, c))
        return x.numpy().astype(np.float64), J.numpy().astype(np.float64)

    @torch.no_grad()
    def module_forward(self, x, c):
        z, J = self.flow.forward(*self._cast(x, c))
        return z.numpy().astype(np.float64), J.numpy().astype(np.float64)

    def set_lr(self, factor):
        if self._fire("lr_dropped", True):
            return
        for grp in self.flow.opt.param_groups:
            grp["lr"] = grp["lr"] * factor

    def repack(self, scale):
        with torch.no_grad():
            for p in self.flow.parameters():
                p.mul_(scale)

    def after_event(self, i, ev):
        pass

    def weights(self):
        return [{k: v.detach().numpy().astype(np.float64) for k, v in P.items()} for P in self.flow.params]

    def moments(self):
        """-> per block {key: (exp_avg, exp_avg_sq)}"""
        st = self.flow.opt.state
        return [{k: (st[v]["exp_avg"].numpy().astype(np.float64), st[v]["exp_avg_sq"].numpy().astype(np.float64))
                 for k, v in P.items()} for P in self.flow.params]


def run_oracle(script: str, flow_name: str, dtype=torch.float64, fault=None, noise=0.0):
    """noise > 0: the session with the training noise on, at that level, keyed by NOISE_SEED"""
    spec = FLOWS[flow_name]
    author = dtype == torch.float64 and fault is None          # the reference run chooses the training rows for all others
    rows = None if author else reference(script, flow_name, noise)["rows"]
    nt = torch.get_num_threads()
    torch.set_num_threads(min(16, nt))
    try:
        be = OracleBackend(spec, dtype, fault, noise)
        rec = run_session(script, spec, be, rows)
    finally:
        torch.set_num_threads(nt)
    rec["initial"] = [{k: v.numpy().astype(np.float64) for k, v in P.items()} for P in be.initial]
    rec["final"] = be.weights()
    rec["moments"] = be.moments()
    rec["dropped"], rec["picked"] = getattr(be, "dropped", 0), getattr(be, "picked", 0)
    return rec


def reference(script: str, flow_name: str, noise=0.0):
    """the float64 oracle's record of a session (cached: the graph and the eager trainer are compared with the same one)"""
    return _reference(script, flow_name, float(noise))


@functools.lru_cache(maxsize=None)
def _reference(script, flow_name, noise):
    return run_oracle(script, flow_name, torch.float64, noise=noise)


# ---- deviations and tolerances ------------------------------------------------------------------------------------------------
def scalar_dev(got, ref) -> float:
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - ref) / (0.1 + np.abs(ref))))


def norm_dev(got, ref) -> float:
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def update_devs(initial, final, final_ref):
    """{(block, key): deviation of the update vector} as check_update of test_gpu_flow.py measures it"""
    return {(bi, k): norm_dev(final[bi][k] - initial[bi][k], final_ref[bi][k] - initial[bi][k])
            for bi in range(len(initial)) for k in initial[bi]}


def deviations(rec, ref):
    """the three compared quantities of a record against the reference record"""
    return dict(losses=scalar_dev(rec["losses"], ref["losses"]), nll=scalar_dev(rec["nll"], ref["nll"]),
                update=max(update_devs(ref["initial"], rec["final"], ref["final"]).values()))


def floors(script: str, flow_name: str, noise=0.0):
    """(noise > 0: the float32 oracle on the same draws - the float32 evaluation of the same Philox outputs, added in float32)"""
    return _floors(script, flow_name, float(noise))


@functools.lru_cache(maxsize=None)
def _floors(script, flow_name, noise):
    return deviations(run_oracle(script, flow_name, torch.float32, noise=noise), reference(script, flow_name, noise))


def tolerances(script: str, flow_name: str, noise=0.0):
    """4 x the float32 oracle's own deviation from the float64 oracle; at least 4 ulp of fp32, at most the existing test's"""
    return {k: min(CAPS[k], 4.0 * max(v, ULP)) for k, v in floors(script, flow_name, noise).items()}


DETECT = 5.0             # an injected fault must move a compared quantity by this many tolerances


@functools.lru_cache(maxsize=None)
def fault_ratios(script: str, flow_name: str, noise: float):
    """{noise fault: (the quantity it moves most, by how many tolerances)} of a noisy session at one level"""
    ref, tol = reference(script, flow_name, noise), tolerances(script, flow_name, noise)
    out = {}
    for fault in NOISE_FAULTS:
        dev = deviations(run_oracle(script, flow_name, fault=fault, noise=noise), ref)
        ratio = {k: dev[k] / tol[k] for k in tol}
        worst = max(ratio, key=ratio.get)
        out[fault] = (worst, ratio[worst])
    return out


@functools.lru_cache(maxsize=None)
def noise_level(script: str, flow_name: str):
    """the level a noisy session runs at: the first of NOISE_LEVELS (the trainers' default 0.01 first) at which every injected
    noise fault moves a compared quantity by DETECT tolerances; None if none does (the CPU calibration test fails then)"""
    for level in NOISE_LEVELS:
        if all(r >= DETECT for _, r in fault_ratios(script, flow_name, level).values()):
            return level
    return None


def adam_factors(lr: float, t: int):
    """what the step prologue leaves in opt_state[3], opt_state[4] for step t, in float64"""
    return lr / (1.0 - BETAS[0] ** t), 1.0 / math.sqrt(1.0 - BETAS[1] ** t)
