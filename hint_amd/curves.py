"""curve_features / lens_forward_process / target_distances / mean_target_distance: the lens-shape simulator of the reference's
evaluation loop on the kernel of hint_curve.hip; trace_fourier_curves / hausdorff_distances / chamfer_distances / lens_fit_loss:
its shape-quality side on the kernel of hint_hausdorff.hip (below, after the simulator); plus_segments / plus_outline_counts /
plus_fit_terms / plus_fit_loss / plus_hausdorff_distances: the plus shape's side on the kernel of hint_plus.hip; lens_fit_grad /
lens_fit_starts / fit_lens_shapes: the lens shape's fit on the kernel of hint_lensfit.hip; plus_fit_grad / plus_dominant_angle /
plus_fit_starts / fit_plus_shapes: the plus shape's fit on the kernel of hint_plusfit.hip; polygon_overlap / lens_iou_dice /
plus_iou_dice: IoU and DICE on the kernel of hint_overlap.hip, and lens_shape_scores / plus_shape_scores: the evaluation loop's
four columns composed of the above (at the end).

    LensShapeModel.forward_process(x, noise=0.05)                      data.py:127-139 (over trace_fourier_curves, data.py:51-57)
    mean_target_distance(model, y_target, x)                           rejection_sampling.py:99-102, called at :204

are a Python loop over rows there - trace the Fourier curve at 100 points, build the 100 x 100 pdist / squareform matrix, take
its argmax - on the CPU, behind a device-to-host copy; here they are one launch of hint_curve_run (two with the mean) that
reads x once and writes y, the distances and their mean, with no host synchronisation.  x is [N, 4K] fp32 in the layout of
flatten_coeffs (data.py:30-40), K odd, 1 <= K <= 25.  The arithmetic and its order are fixed (include/hint_amd.h), so a row's
result does not depend on the batch and two runs agree bit for bit.  The reference draws its noise from numpy's global
generator; here eps is an argument, or torch.randn on the device.  No gradient is implemented and there is no CPU fallback.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import torch

from . import _lib
from ._lib import HintAmdError
from ._ops import _check_no_grad, _check_real, _outputs, _run_desc

__all__ = ["curve_features", "lens_forward_process", "target_distances", "mean_target_distance",
           "trace_fourier_curves", "hausdorff_distances", "chamfer_distances", "lens_fit_loss",
           "plus_segments", "plus_outline_counts", "plus_fit_terms", "plus_fit_loss", "plus_hausdorff_distances",
           "lens_fit_grad", "lens_fit_starts", "fit_lens_shapes",
           "plus_fit_grad", "plus_dominant_angle", "plus_fit_starts", "fit_plus_shapes",
           "polygon_overlap", "lens_iou_dice", "plus_iou_dice", "lens_shape_scores", "plus_shape_scores"]

MAX_COEFFS = 25
MIN_POINTS, MAX_POINTS = 2, 128
MAX_ROWS = 1 << 30


def _check_x(x, who: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        raise HintAmdError(f"{who}: x must be a tensor (got {type(x).__name__})")
    if x.dim() != 2:
        raise HintAmdError(f"{who}: x must be 2-D [rows, 4 K coefficients] (got shape {tuple(x.shape)})")
    if not x.is_cuda:
        raise HintAmdError(f"{who}: x is on {x.device}; the simulator is a GPU kernel and there is no CPU fallback")
    if not x.is_floating_point():
        raise HintAmdError(f"{who}: x is {x.dtype}; expected a floating-point tensor")
    _check_shape(tuple(x.shape), who)
    x = x.detach()
    if x.dtype != torch.float32 or not x.is_contiguous():          # (copies only where needed)
        x = x.to(torch.float32).contiguous()
    return x


def _check_shape(shape, who: str) -> int:
    n, c = shape
    if n < 1 or n > MAX_ROWS:
        raise HintAmdError(f"{who}: x must hold 1..{MAX_ROWS} rows (got shape {shape})")
    if c % 4 != 0 or (c // 4) % 2 != 1 or c // 4 > MAX_COEFFS:
        raise HintAmdError(f"{who}: x must hold 4 K columns with K odd, 1..{MAX_COEFFS} (got shape {shape})")
    return c // 4


def _check_points(v, who: str, most: int = MAX_POINTS) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise HintAmdError(f"{who}: n_points must be an int (got {type(v).__name__})")
    if v < MIN_POINTS or v > most:
        raise HintAmdError(f"{who}: n_points must be {MIN_POINTS}..{most} (got {v})")
    return v


def _check_weight(v, name: str, who: str) -> float:
    """the weight of a loss's second term: any number but NaN (an infinite one included)"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
        raise HintAmdError(f"{who}: {name} must be a number (got {v!r})")
    return float(v)


def _check_target(target, n_rows: int, device, who: str) -> torch.Tensor:
    """[2], [1, 2], or - as the reference passes it (rejection_sampling.py:195, :101) - expanded to [N, 2], of which row 0 counts"""
    try:
        t = target if isinstance(target, torch.Tensor) else torch.as_tensor(target)
    except (TypeError, ValueError, RuntimeError) as e:
        raise HintAmdError(f"{who}: y_target must be a tensor or an array-like of 2 numbers: {e}") from e
    if tuple(t.shape) not in ((2,), (1, 2), (n_rows, 2)):
        raise HintAmdError(f"{who}: y_target must have shape [2], [1, 2] or [{n_rows}, 2] (got {tuple(t.shape)})")
    if t.dim() == 2:
        t = t[0]
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _check_eps(eps, x: torch.Tensor, who: str) -> torch.Tensor:
    if not isinstance(eps, torch.Tensor):
        raise HintAmdError(f"{who}: eps must be a tensor (got {type(eps).__name__})")
    if tuple(eps.shape) != (x.shape[0], 2):
        raise HintAmdError(f"{who}: eps must have shape [{x.shape[0]}, 2] (got {tuple(eps.shape)})")
    if eps.device != x.device:
        raise HintAmdError(f"{who}: eps is on {eps.device} and x on {x.device}")
    return eps.detach().to(torch.float32).contiguous()


def _noise_args(x: torch.Tensor, noise, eps, generator, who: str):
    noise = _check_real(noise, "noise", who, nonneg=False)
    if eps is not None:
        return noise, _check_eps(eps, x, who)
    if noise == 0.0:
        return 0.0, None
    if generator is not None and not isinstance(generator, torch.Generator):
        raise HintAmdError(f"{who}: generator must be a torch.Generator (got {type(generator).__name__})")
    return noise, torch.randn(x.shape[0], 2, device=x.device, dtype=torch.float32, generator=generator)


def _set_curve(desc, curve: Optional[torch.Tensor], n: int, k: int, p: int):
    """the descriptor's rows and curve source: curve [N, 4K] coefficients traced at p points, or (k = 0) [N, p, 2] points; None:
    the call reads no curve"""
    if curve is not None:
        desc.x, desc.b_points = (curve.data_ptr(), None) if k else (None, curve.data_ptr())
    desc.n_rows, desc.n_coeffs, desc.n_points = n, k, p


_F32, _I32 = torch.float32, torch.int32


def _run(x: torch.Tensor, n_points: int, eps: Optional[torch.Tensor] = None, noise: float = 0.0,
         target: Optional[torch.Tensor] = None, want_dist: bool = False, want_mean: bool = False, max_groups: int = 0):
    """one hint_curve_run on checked arguments: (y [N, 2], dist [N] or None, mean 0-dim or None)"""
    n, c = x.shape
    desc = _lib.CurveDesc()
    desc.x, desc.n_rows, desc.n_coeffs, desc.n_points = x.data_ptr(), n, c // 4, n_points
    desc.eps, desc.noise = (eps.data_ptr() if eps is not None else None), noise
    desc.target = target.data_ptr() if target is not None else None
    want = ["y"]
    if want_dist:
        want.append("dist")
    if want_mean:
        want.append("mean")
    res = _outputs(desc, dict(y=((n, 2), _F32), dist=((n,), _F32), mean=((), _F32)), want, None, x.device)
    desc.max_groups = max_groups
    _run_desc("hint_curve_run", desc, x.device, (n, c // 4, n_points) if want_mean else None)      # (only the mean needs a workspace)
    return res["y"], res.get("dist"), res.get("mean")


def curve_features(x: torch.Tensor, n_points: int = 100) -> torch.Tensor:
    """the simulator without noise: for each row of x [N, 4K] the vector between the two curve points farthest apart, as
    (dy, dx) - forward_process(x, noise=0) of the reference - [N, 2] fp32 on x's device"""
    who = "curve_features"
    x = _check_x(x, who)
    return _run(x, _check_points(n_points, who))[0]


def lens_forward_process(x: torch.Tensor, noise: float = 0.05, *, eps: Optional[torch.Tensor] = None,
                         generator: Optional[torch.Generator] = None, n_points: int = 100) -> torch.Tensor:
    """the reference's LensShapeModel.forward_process(x, noise): curve_features(x) + noise * eps, eps [N, 2] given or drawn with
    torch.randn on x's device (from generator, if one is given); noise = 0 without eps is curve_features"""
    who = "lens_forward_process"
    x = _check_x(x, who)
    n_points = _check_points(n_points, who)
    noise, eps = _noise_args(x, noise, eps, generator, who)
    return _run(x, n_points, eps, noise)[0]


def target_distances(x: torch.Tensor, y_target, noise: float = 0.05, *, eps: Optional[torch.Tensor] = None,
                     generator: Optional[torch.Generator] = None, n_points: int = 100) -> torch.Tensor:
    """|lens_forward_process(x, noise) - y_target| per row, [N] fp32"""
    who = "target_distances"
    x = _check_x(x, who)
    n_points = _check_points(n_points, who)
    t = _check_target(y_target, x.shape[0], x.device, who)
    noise, eps = _noise_args(x, noise, eps, generator, who)
    return _run(x, n_points, eps, noise, t, want_dist=True)[1]


def mean_target_distance(x: torch.Tensor, y_target, noise: float = 0.05, *, eps: Optional[torch.Tensor] = None,
                         generator: Optional[torch.Generator] = None, n_points: int = 100) -> torch.Tensor:
    """the reference's mean_target_distance(model, y_target, x) for the lens-shape model: the mean of target_distances, summed in
    double in a fixed order, a 0-dim fp32 tensor on x's device.  y_target may be [2], [1, 2] or, as the reference passes it,
    already expanded to [N, 2] (row 0 counts)"""
    who = "mean_target_distance"
    x = _check_x(x, who)
    n_points = _check_points(n_points, who)
    t = _check_target(y_target, x.shape[0], x.device, who)
    noise, eps = _noise_args(x, noise, eps, generator, who)
    return _run(x, n_points, eps, noise, t, want_mean=True)[2]


# ---- dense tracing and the distances of a curve to a template (hint_hausdorff.hip) ----
#     trace_fourier_curves(coeffs, n_points)                             data.py:51-57
#     max_and_avg_hausdorff_distance(template, dense_curve)              best_shape_fit.py:143-149, per row at run_experiments.py:147-159
#     lens_points_from_params(prototype, params)                         best_shape_fit.py:195-199
#     points_to_lens_loss(prototype, points, params, lens_fit_weight)    best_shape_fit.py:203-209
# One launch of hint_hausdorff_run per call: no [N, P, M] tensor, no host synchronisation, the arithmetic and the order of the sums
# fixed (include/hint_amd.h).  The shape fits and IoU / DICE follow below; the template generators stay on the host.
MAX_DENSE_POINTS = 1024
MAX_TEMPLATE_POINTS = 4096


def _check_dense_points(v, who: str) -> int:
    return _check_points(v, who, MAX_DENSE_POINTS)


def _check_dev_tensor(t, name: str, who: str, device=None) -> torch.Tensor:
    """a floating-point tensor on the GPU (on `device`, if given) that no gradient is asked of -> detached, fp32, contiguous"""
    if not isinstance(t, torch.Tensor):
        raise HintAmdError(f"{who}: {name} must be a tensor (got {type(t).__name__})")
    if not t.is_cuda:
        raise HintAmdError(f"{who}: {name} is on {t.device}; the distances are a GPU kernel and there is no CPU fallback")
    if device is not None and t.device != device:
        raise HintAmdError(f"{who}: {name} is on {t.device} and curve on {device}")
    if not t.is_floating_point():
        raise HintAmdError(f"{who}: {name} is {t.dtype}; expected a floating-point tensor")
    _check_no_grad(t, name, who)
    t = t.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():              # (copies only where needed)
        t = t.to(torch.float32).contiguous()
    return t


def _check_curve_shape(shape, n_points, who: str):
    """(rows, K or 0, P) of curve [N, 4K] (coefficients, traced at n_points) or [N, P, 2] (points; n_points is not looked at)"""
    if len(shape) == 2:
        return shape[0], _check_shape(tuple(shape), who), _check_dense_points(n_points, who)
    if len(shape) != 3 or shape[2] != 2:
        raise HintAmdError(f"{who}: curve must be [rows, 4 K] coefficients or [rows, P, 2] points (got shape {tuple(shape)})")
    n, p = shape[0], shape[1]
    if n < 1 or n > MAX_ROWS:
        raise HintAmdError(f"{who}: curve must hold 1..{MAX_ROWS} rows (got shape {tuple(shape)})")
    if p < MIN_POINTS or p > MAX_DENSE_POINTS:
        raise HintAmdError(f"{who}: curve must hold {MIN_POINTS}..{MAX_DENSE_POINTS} points a row (got shape {tuple(shape)})")
    return n, 0, p


def _check_template_shape(shape, ragged: bool, who: str) -> int:
    if len(shape) != 2 or shape[1] != 2:
        raise HintAmdError(f"{who}: template must be [points, 2] (got shape {tuple(shape)})")
    if shape[0] < 1:
        raise HintAmdError(f"{who}: template is empty (shape {tuple(shape)})")
    if not ragged and shape[0] > MAX_TEMPLATE_POINTS:
        raise HintAmdError(f"{who}: a shared template must hold 1..{MAX_TEMPLATE_POINTS} points (got {shape[0]}); per-row "
                           "templates go through offsets")
    return shape[0]


def _check_offsets(offsets, n_rows: int, n_template: int, who: str) -> torch.Tensor:
    """offsets as int64 [n_rows + 1].  Values on the host (a CPU tensor, an array, a list) are checked here: ascending from 0 to
    the template's points, 1..4096 points a row.  A tensor that is on the GPU already is not read back - the kernel gives a row
    with a bad range NaN."""
    try:
        o = offsets if isinstance(offsets, torch.Tensor) else torch.as_tensor(offsets)
    except (TypeError, ValueError, RuntimeError) as e:
        raise HintAmdError(f"{who}: offsets must be a tensor or an array-like of integers: {e}") from e
    if o.is_floating_point() or o.is_complex() or o.dtype == torch.bool:
        raise HintAmdError(f"{who}: offsets is {o.dtype}; expected an integer tensor")
    if tuple(o.shape) != (n_rows + 1,):
        raise HintAmdError(f"{who}: offsets must have shape [{n_rows + 1}] (rows + 1; got {tuple(o.shape)})")
    if o.is_cuda:
        return o.detach().to(torch.int64).contiguous()
    o = o.detach().to(torch.int64).contiguous()
    if int(o[0]) != 0 or int(o[-1]) != n_template:
        raise HintAmdError(f"{who}: offsets must ascend from 0 to the template's {n_template} points "
                           f"(got {int(o[0])} .. {int(o[-1])})")
    d = o[1:] - o[:-1]
    if int(d.min()) < 1 or int(d.max()) > MAX_TEMPLATE_POINTS:
        r = int(((d < 1) | (d > MAX_TEMPLATE_POINTS)).nonzero()[0])
        raise HintAmdError(f"{who}: offsets must ascend by 1..{MAX_TEMPLATE_POINTS} points a row (row {r}: {int(d[r])})")
    return o


def _check_params_shape(shape, n_rows: int, who: str):
    if tuple(shape) not in ((4,), (1, 4), (n_rows, 4)):
        raise HintAmdError(f"{who}: params must have shape [4], [1, 4] or [{n_rows}, 4]: x, y, scale, angle "
                           f"(got {tuple(shape)})")


def _curve_arg(curve, n_points, who: str):
    """curve, as [N, 4K] coefficients or [N, P, 2] points -> (the checked device tensor, rows, K or 0, P)"""
    if not isinstance(curve, torch.Tensor):
        raise HintAmdError(f"{who}: curve must be a tensor (got {type(curve).__name__})")
    if curve.dim() not in (2, 3):
        raise HintAmdError(f"{who}: curve must be [rows, 4 K] coefficients or [rows, P, 2] points (got shape {tuple(curve.shape)})")
    curve = _check_dev_tensor(curve, "curve", who)
    return (curve,) + _check_curve_shape(tuple(curve.shape), n_points, who)


def _distance_args(curve, template, params, offsets, n_points, who: str):
    curve, n, k, p = _curve_arg(curve, n_points, who)
    template = _check_dev_tensor(template, "template", who, curve.device)
    t_pts = _check_template_shape(tuple(template.shape), offsets is not None, who)
    if offsets is not None:
        offsets = _check_offsets(offsets, n, t_pts, who).to(curve.device)
    if params is not None:
        params = _check_dev_tensor(params, "params", who, curve.device)
        _check_params_shape(tuple(params.shape), n, who)
        params = params.reshape(-1, 4).expand(n, 4).contiguous()
    return curve, k, p, template, offsets, params


def _hd_run(curve: torch.Tensor, k: int, p: int, template: Optional[torch.Tensor], offsets: Optional[torch.Tensor] = None,
            params: Optional[torch.Tensor] = None, want_h: bool = False, want_chamfer: bool = False, want_points: bool = False,
            max_groups: int = 0):
    """one hint_hausdorff_run on checked arguments: (max_h [N], avg_h [N], chamfer [N, 2], points [N, P, 2]), None where not asked.
    k = 0: curve is [N, P, 2] points.  template None (points alone): the kernel then reads no template, and the descriptor names
    the first two floats of curve as one"""
    n, dev = curve.shape[0], curve.device
    desc = _lib.HausdorffDesc()
    _set_curve(desc, curve, n, k, p)
    desc.a_points = template.data_ptr() if template is not None else curve.data_ptr()
    desc.n_template = template.shape[0] if template is not None else 1
    desc.a_offsets = offsets.data_ptr() if offsets is not None else None
    desc.a_params = params.data_ptr() if params is not None else None
    want = []
    if want_h:
        want += ["max_h", "avg_h"]
    if want_chamfer:
        want.append("chamfer")
    if want_points:
        want.append("points")
    res = _outputs(desc, dict(max_h=((n,), _F32), avg_h=((n,), _F32), chamfer=((n, 2), _F32), points=((n, p, 2), _F32)), want, None, dev)
    desc.max_groups = max_groups
    _run_desc("hint_hausdorff_run", desc, dev)
    return res.get("max_h"), res.get("avg_h"), res.get("chamfer"), res.get("points")


def trace_fourier_curves(x: torch.Tensor, n_points: int = 100) -> torch.Tensor:
    """the reference's data_model.trace_fourier_curves(unflatten_coeffs(x), n_points) on flat x [N, 4K]: the curve's points
    [N, n_points, 2] fp32 on x's device, 2 <= n_points <= 1024; the last point repeats the first bit for bit.  Up to 128 points
    these are the points curve_features measures"""
    who = "trace_fourier_curves"
    if isinstance(x, torch.Tensor):
        _check_no_grad(x, "x", who)
    x = _check_x(x, who)
    return _hd_run(x, x.shape[1] // 4, _check_dense_points(n_points, who), None, want_points=True)[3]


def hausdorff_distances(curve: torch.Tensor, template: torch.Tensor, params: Optional[torch.Tensor] = None, *, offsets=None,
                        n_points: int = 1000):
    """the reference's max_and_avg_hausdorff_distance(template, dense curve) for every row: (max_h [N], avg_h [N]) fp32.

    curve     [N, 4K] coefficients, traced at n_points here, or [N, P, 2] points (n_points is then ignored)
    template  [M, 2], M <= 4096, shared by all rows; or, with offsets (int64 [N + 1], ascending from 0 to T, on the host or the
              device), [T, 2] of which row n owns template[offsets[n]:offsets[n + 1]], 1..4096 points
    params    None, or [N, 4] (or [4]) = x, y, scale, angle: the template is first moved as lens_points_from_params does"""
    who = "hausdorff_distances"
    curve, k, p, template, offsets, params = _distance_args(curve, template, params, offsets, n_points, who)
    return _hd_run(curve, k, p, template, offsets, params, want_h=True)[:2]


def chamfer_distances(curve: torch.Tensor, template: torch.Tensor, params: Optional[torch.Tensor] = None, *, offsets=None,
                      n_points: int = 1000) -> torch.Tensor:
    """[N, 2] fp32: per row (the mean over the curve's points of the squared distance to the nearest template point, the mean
    over the template's points of the squared distance to the nearest curve point).  Arguments as hausdorff_distances (n_points
    is ignored when curve holds points)"""
    who = "chamfer_distances"
    curve, k, p, template, offsets, params = _distance_args(curve, template, params, offsets, n_points, who)
    return _hd_run(curve, k, p, template, offsets, params, want_chamfer=True)[2]


def lens_fit_loss(curve: torch.Tensor, prototype: torch.Tensor, params: torch.Tensor, lens_fit_weight: float = 1.0) -> torch.Tensor:
    """the reference's points_to_lens_loss(prototype, points, params, lens_fit_weight) for every row, [N] fp32:
    chamfer[:, 0] + lens_fit_weight * chamfer[:, 1] of chamfer_distances(curve, prototype, params).  curve as in
    hausdorff_distances; coefficients are traced at 100 points, as the fit's points are"""
    who = "lens_fit_loss"
    weight = _check_weight(lens_fit_weight, "lens_fit_weight", who)
    if params is None:
        raise HintAmdError(f"{who}: params must be a tensor (got None)")
    curve, k, p, prototype, _, params = _distance_args(curve, prototype, params, None, 100, who)
    ch = _hd_run(curve, k, p, prototype, None, params, want_chamfer=True)[2]
    return ch[:, 0] + weight * ch[:, 1]


# ---- the plus shape: outline, fit loss and distances to the densified outline (hint_plus.hip) ----
#     plus_segments_from_params(params)                                  best_shape_fit.py:26-50
#     points_to_plus_loss(points, params, corner_weight)                 best_shape_fit.py:54-65 (over :15-22)
#     max_and_avg_hausdorff_distance_plus_shape(params, points)          best_shape_fit.py:153-156, per row at eval_shapes.py:82-95
#     PlusShapeModel.densify_polyline(coords, max_dist)                  data.py:176-186
# One launch of hint_plus_run per call.  The outline's points are generated inside the kernel: no template is built or uploaded
# and there is no per-row host work.  The fit itself (fit_plus_shape_to_points) is fit_plus_shapes and IoU / DICE plus_iou_dice,
# at the end.
PLUS_PARAMS = 9
MAX_OUTLINE_POINTS = 4096


def _check_max_dist(v, who: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise HintAmdError(f"{who}: max_dist must be a number (got {type(v).__name__})")
    v = float(v)
    if not (v > 0.0) or v == float("inf"):
        raise HintAmdError(f"{who}: max_dist must be finite and > 0 (got {v})")
    return v


def _check_plus_params_shape(shape, n_rows: Optional[int], who: str) -> None:
    """[9], [1, 9] or [n_rows, 9]; n_rows None: the params alone decide the rows ([9] or [N, 9], N >= 1)"""
    shape = tuple(shape)
    if n_rows is None:
        if shape == (PLUS_PARAMS,) or (len(shape) == 2 and shape[1] == PLUS_PARAMS and 1 <= shape[0] <= MAX_ROWS):
            return
        raise HintAmdError(f"{who}: params must have shape [9] or [rows, 9]: xlength, ylength, xwidth, ywidth, xshift, yshift, "
                           f"xoffset, yoffset, angle (got {shape})")
    if shape not in ((PLUS_PARAMS,), (1, PLUS_PARAMS), (n_rows, PLUS_PARAMS)):
        raise HintAmdError(f"{who}: params must have shape [9], [1, 9] or [{n_rows}, 9]: xlength, ylength, xwidth, ywidth, "
                           f"xshift, yshift, xoffset, yoffset, angle (got {shape})")


def _plus_params(params, n_rows: Optional[int], who: str, device=None) -> torch.Tensor:
    params = _check_dev_tensor(params, "params", who, device)
    _check_plus_params_shape(tuple(params.shape), n_rows, who)
    params = params.reshape(-1, PLUS_PARAMS)
    if n_rows is not None and params.shape[0] != n_rows:
        params = params.expand(n_rows, PLUS_PARAMS)
    return params.contiguous()


def _plus_args(curve, params, n_points, who: str):
    curve, n, k, p = _curve_arg(curve, n_points, who)
    return curve, k, p, _plus_params(params, n, who, curve.device)


def _plus_run(params: torch.Tensor, curve: Optional[torch.Tensor] = None, k: int = 0, p: int = 0, max_dist: float = 0.02,
              want=("segments", "keep", "counts", "loss", "max_h", "avg_h"), max_groups: int = 0, out=None):
    """one hint_plus_run on checked arguments: a dict of the outputs named in `want` (segments [N, 12, 2, 2], keep [N] int32,
    counts [N, 12] int32, loss [N, 2], max_h [N], avg_h [N]).  k = 0: curve is [N, P, 2] points; curve None: no curve output.
    out: tensors to write into instead of new ones (the tests' guarded buffers)"""
    n, dev = params.shape[0], params.device
    desc = _lib.PlusDesc()
    _set_curve(desc, curve, n, k, p)
    desc.params, desc.max_dist, desc.max_groups = params.data_ptr(), max_dist, max_groups
    res = _outputs(desc, dict(segments=((n, 12, 2, 2), _F32), keep=((n,), _I32), counts=((n, 12), _I32), loss=((n, 2), _F32),
                              max_h=((n,), _F32), avg_h=((n,), _F32)), want, out, dev)
    _run_desc("hint_plus_run", desc, dev)
    return res


def plus_segments(params: torch.Tensor):
    """the reference's plus_segments_from_params(params) for every row of params [N, 9] (or [9]) = xlength, ylength, xwidth,
    ywidth, xshift, yshift, xoffset, yoffset, angle: (segments [N, 12, 2, 2] fp32 - all twelve, placed - and keep [N] int32, whose
    bit s says that the reference keeps segment s; it drops those of zero length, which only a zero width gives)"""
    who = "plus_segments"
    res = _plus_run(_plus_params(params, None, who), want=("segments", "keep"))
    return res["segments"], res["keep"]


def plus_outline_counts(params: torch.Tensor, max_dist: float = 0.02) -> torch.Tensor:
    """[N, 12] int32: the points densify_polyline(outline, max_dist) puts on each edge - 0 for a dropped segment; -1 in every
    column of a row whose outline cannot be served (more than 4096 points, parameters that are not finite)"""
    who = "plus_outline_counts"
    max_dist = _check_max_dist(max_dist, who)
    return _plus_run(_plus_params(params, None, who), max_dist=max_dist, want=("counts",))["counts"]


def plus_fit_terms(curve: torch.Tensor, params: torch.Tensor, *, n_points: int = 100) -> torch.Tensor:
    """[N, 2] fp32: the two terms of the reference's points_to_plus_loss per row - the mean over the curve's points of the squared
    distance to the nearest outline segment, and the mean over the outline's corners of the squared distance to the nearest curve
    point.  curve is [N, 4K] coefficients, traced at n_points here, or [N, P, 2] points (n_points is then ignored); params [N, 9],
    [1, 9] or [9]"""
    who = "plus_fit_terms"
    curve, k, p, params = _plus_args(curve, params, n_points, who)
    return _plus_run(params, curve, k, p, want=("loss",))["loss"]


def plus_fit_loss(curve: torch.Tensor, params: torch.Tensor, corner_weight: float = 1.0) -> torch.Tensor:
    """the reference's points_to_plus_loss(points, params, corner_weight) for every row, [N] fp32: terms[:, 0] + corner_weight *
    terms[:, 1] of plus_fit_terms.  Coefficients are traced at 100 points, as the fit's points are"""
    who = "plus_fit_loss"
    weight = _check_weight(corner_weight, "corner_weight", who)
    curve, k, p, params = _plus_args(curve, params, 100, who)
    terms = _plus_run(params, curve, k, p, want=("loss",))["loss"]
    return terms[:, 0] + weight * terms[:, 1]


def plus_hausdorff_distances(curve: torch.Tensor, params: torch.Tensor, *, max_dist: float = 0.02, n_points: int = 1000):
    """the reference's max_and_avg_hausdorff_distance_plus_shape(params, dense curve) for every row: (max_h [N], avg_h [N]) fp32
    between the curve and the outline densified at max_dist.  curve and params as in plus_fit_terms.  A row whose outline would
    hold more than 4096 points, or whose parameters are not finite, gets NaN in both"""
    who = "plus_hausdorff_distances"
    max_dist = _check_max_dist(max_dist, who)
    curve, k, p, params = _plus_args(curve, params, n_points, who)
    res = _plus_run(params, curve, k, p, max_dist, want=("max_h", "avg_h"))
    return res["max_h"], res["avg_h"]


# ---- the lens shape's fit: loss, gradient and the SGD loop over the starts in one launch (hint_lensfit.hip) ----
#     fit_lens_shape_to_points(points)                                   best_shape_fit.py:230-261, per row at run_experiments.py:150-159
#     points_to_lens_loss(prototype, points, params, w).backward()       best_shape_fit.py:203-209 (over :195-199)
# One launch of hint_lensfit_run per call: no [N, S, P, M] tensor, no autograd graph, no per-row host work; the arithmetic, the
# selected pairs, the order of the sums and the update rule are fixed (include/hint_amd.h).  The plus shape's fit follows below.
MAX_PROTOTYPE_POINTS = 1024
MAX_STARTS = 16
MAX_FIT_STEPS = 1024
FIT_POINTS = 100           # the points a curve given as coefficients is traced at (run_experiments.py:147)


def _check_steps(v, who: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise HintAmdError(f"{who}: n_steps must be an int (got {type(v).__name__})")
    if v < 0 or v > MAX_FIT_STEPS:
        raise HintAmdError(f"{who}: n_steps must be 0..{MAX_FIT_STEPS} (got {v})")
    return v


def _check_prototype_shape(shape, who: str) -> int:
    if len(shape) != 2 or shape[1] != 2:
        raise HintAmdError(f"{who}: prototype must be [points, 2] (got shape {tuple(shape)})")
    if shape[0] < 1 or shape[0] > MAX_PROTOTYPE_POINTS:
        raise HintAmdError(f"{who}: prototype must hold 1..{MAX_PROTOTYPE_POINTS} points (got shape {tuple(shape)})")
    return shape[0]


def _check_starts_shape(shape, n_rows: int, who: str) -> int:
    shape = tuple(shape)
    if len(shape) != 3 or shape[0] != n_rows or shape[2] != 4 or not 1 <= shape[1] <= MAX_STARTS:
        raise HintAmdError(f"{who}: starts must have shape [{n_rows}, S, 4] with S 1..{MAX_STARTS}: x, y, scale, angle "
                           f"(got {shape})")
    return shape[1]


def _fit_args(curve, prototype, who: str):
    curve, n, k, p = _curve_arg(curve, FIT_POINTS, who)
    prototype = _check_dev_tensor(prototype, "prototype", who, curve.device)
    _check_prototype_shape(tuple(prototype.shape), who)
    return curve, n, k, p, prototype


def _fit_run(desc_cls, entry: str, n_params: int, fields: dict, curve: torch.Tensor, k: int, p: int, starts: torch.Tensor,
             n_steps: int, lr: float, angle_lr: float, gamma: float, momentum: float, want, max_groups: int, out):
    """one run of a fit's entry point on checked arguments, what _lf_run and _pf_run share: a dict of the outputs named in `want`.
    fields: the descriptor's fields beside the curve, the starts and the schedule (a trace record is 2 n_params + 1 floats)"""
    n, dev, s = curve.shape[0], curve.device, starts.shape[1]
    desc = desc_cls()
    _set_curve(desc, curve, n, k, p)
    desc.starts, desc.n_starts, desc.n_steps = starts.data_ptr(), s, n_steps
    desc.lr, desc.angle_lr, desc.gamma, desc.momentum = lr, angle_lr, gamma, momentum
    for name, v in fields.items():
        setattr(desc, name, v)
    table = dict(params=((n, n_params), _F32), loss=((n,), _F32), best=((n,), _I32), all_params=((n, s, n_params), _F32),
                 all_loss=((n, s), _F32), grad=((n, s, n_params), _F32), trace=((n, s, n_steps, 2 * n_params + 1), _F32))
    if hasattr(desc, "n_run"):
        table["n_run"] = ((n,), _I32)
    res = _outputs(desc, table, want, out, dev)
    desc.max_groups = max_groups
    _run_desc(entry, desc, dev)
    return res


def _check_schedule(n_steps, lr, angle_lr, momentum, gamma, weight, weight_name: str, who: str):
    """a fit's n_steps, lr, angle_lr, momentum, gamma and weight, checked in this order"""
    return (_check_steps(n_steps, who), _check_real(lr, "lr", who), _check_real(angle_lr, "angle_lr", who),
            _check_real(momentum, "momentum", who), _check_real(gamma, "gamma", who),
            _check_real(weight, weight_name, who, nonneg=False))


def _fit_result(run, starts: torch.Tensor, n_steps: int, return_all: bool, return_trace: bool, extra=()):
    """what a fit returns, from run(want) -> the dict of the outputs named in want: (params, loss) and, with return_all or
    return_trace, a dict of the others (best and `extra`; all_params, all_loss; trace, empty for n_steps = 0)"""
    want = ["params", "loss"]
    if return_all or return_trace:
        want += ["best", *extra]
    if return_all:
        want += ["all_params", "all_loss"]
    if return_trace and n_steps > 0:
        want.append("trace")
    res = run(tuple(want))
    if not (return_all or return_trace):
        return res["params"], res["loss"]
    if return_trace and n_steps == 0:
        res["trace"] = torch.empty(*starts.shape[:2], 0, 2 * starts.shape[2] + 1, dtype=torch.float32, device=starts.device)
    return res["params"], res["loss"], {name: v for name, v in res.items() if name not in ("params", "loss")}


def _lf_run(curve: torch.Tensor, k: int, p: int, prototype: torch.Tensor, starts: torch.Tensor, n_steps: int = 0, lr: float = 0.1,
            angle_lr: float = 0.01, gamma: float = 1.0, momentum: float = 0.0, weight: float = 1.0,
            want=("params", "loss", "best", "all_params", "all_loss", "grad"), max_groups: int = 0, out=None):
    """one hint_lensfit_run on checked arguments: a dict of the outputs named in `want` (params [N, 4], loss [N], best [N] int32,
    all_params [N, S, 4], all_loss [N, S], grad [N, S, 4], trace [N, S, n_steps, 9]).  k = 0: curve is [N, P, 2] points.
    out: tensors to write into instead of new ones (the tests' guarded buffers)"""
    fields = dict(a_points=prototype.data_ptr(), n_template=prototype.shape[0], weight=weight)
    return _fit_run(_lib.LensFitDesc, "hint_lensfit_run", 4, fields, curve, k, p, starts, n_steps, lr, angle_lr, gamma, momentum,
                    want, max_groups, out)


def lens_fit_grad(curve: torch.Tensor, prototype: torch.Tensor, params: torch.Tensor, lens_fit_weight: float = 1.0):
    """the reference's points_to_lens_loss(prototype, points, params, lens_fit_weight) and its autograd gradient by the four
    parameters, for every row: (loss [N], grad [N, 4]) fp32 - one launch, no autograd graph.  curve is [N, 4K] coefficients,
    traced at 100 points as the fit's points are, or [N, P, 2] points; prototype [M, 2], M <= 1024; params [N, 4], [1, 4] or [4] =
    x, y, scale, angle.  Where two prototype (or curve) points are equally near, the gradient is the one of the first"""
    who = "lens_fit_grad"
    weight = _check_real(lens_fit_weight, "lens_fit_weight", who, nonneg=False)
    if params is None:
        raise HintAmdError(f"{who}: params must be a tensor (got None)")
    curve, n, k, p, prototype = _fit_args(curve, prototype, who)
    params = _check_dev_tensor(params, "params", who, curve.device)
    _check_params_shape(tuple(params.shape), n, who)
    starts = params.reshape(-1, 4).expand(n, 4).reshape(n, 1, 4).contiguous()
    res = _lf_run(curve, k, p, prototype, starts, 0, weight=weight, want=("all_loss", "grad"))
    return res["all_loss"].reshape(n), res["grad"].reshape(n, 4)


def _tree_sum(v: torch.Tensor) -> torch.Tensor:
    """the sum of v [n, p, ...] over its second axis as a pairwise tree of elementwise sums (the count padded to a power of two
    with zeros): a row's bits do not depend on the batch, as a library reduction's might"""
    n, p = v.shape[0], v.shape[1]
    width = 1 << (p - 1).bit_length() if p > 1 else 1
    acc = torch.zeros((n, width) + tuple(v.shape[2:]), dtype=v.dtype, device=v.device)
    acc[:, :p] = v
    while width > 1:
        width //= 2
        acc = acc[:, :width] + acc[:, width:]
    return acc[:, 0]


def lens_fit_starts(curve: torch.Tensor) -> torch.Tensor:
    """[N, 2, 4] fp32: the two starts (x, y, scale, angle) of the reference's fit_lens_shape_to_points for every row, computed on
    the device - the centre is the mean of the curve's points (a traced curve's repeated end point included), the scale 2, the
    angle -atan2(dx, dy) of the vector between the two points farthest apart (the first such pair in row-major order) and
    (angle + pi) mod 2 pi.  curve is [N, 4K] coefficients, traced at 100 points, or [N, P, 2] points (plain torch on the [P, P]
    distances then, at most 2^24 of them at a time).  A row that holds a value that is not finite gets unspecified starts; no
    index comes from it and no other row is touched"""
    who = "lens_fit_starts"
    curve, n, k, p = _curve_arg(curve, FIT_POINTS, who)
    if k:
        f = _run(curve, p)[0]                                                 # (dy, dx) of curve_features' pair
        pts = _hd_run(curve, k, p, None, want_points=True)[3]
        dy, dx = f[:, 0], f[:, 1]
    else:
        pts = curve
        # the first maximum of the [P, P] squared distances in row-major order, rows in chunks so that no more than 2^24 of them
        # exist at a time.  A distance that is not a number counts as -1: the index is then always one of the row's own pairs,
        # whatever the row holds
        v = torch.empty(n, 2, dtype=torch.float32, device=curve.device)
        flat = torch.arange(p * p, device=curve.device)
        step = max(1, (1 << 24) // (p * p))
        for a in range(0, n, step):
            c = pts[a:a + step]
            ddx, ddy = c[:, :, None, 0] - c[:, None, :, 0], c[:, :, None, 1] - c[:, None, :, 1]
            d2 = torch.nan_to_num(ddx * ddx + ddy * ddy, nan=-1.0).reshape(c.shape[0], p * p)
            first = torch.where(d2 == d2.amax(1, keepdim=True), flat, p * p).amin(1).clamp_(max=p * p - 1)
            rows = torch.arange(c.shape[0], device=curve.device)
            v[a:a + step] = c[rows, first % p] - c[rows, first // p]
        dx, dy = v[:, 0], v[:, 1]
    angle = -torch.atan2(dx, dy)
    second = torch.remainder(angle + torch.pi, 2 * torch.pi)
    centre = _tree_sum(pts) / p
    out = torch.empty(n, 2, 4, dtype=torch.float32, device=curve.device)
    out[:, :, 0:2] = centre[:, None, :]
    out[:, :, 2] = 2.0
    out[:, 0, 3] = angle
    out[:, 1, 3] = second
    return out


def fit_lens_shapes(curve: torch.Tensor, prototype: torch.Tensor, *, starts: Optional[torch.Tensor] = None, n_steps: int = 100,
                    lr: float = 0.1, angle_lr: float = 0.01, momentum: float = 0.2, gamma: float = 0.1 ** (1 / 100),
                    lens_fit_weight: float = 1.0, return_all: bool = False, return_trace: bool = False):
    """the reference's fit_lens_shape_to_points for every row in one launch: from each of the row's starts (lens_fit_starts(curve)
    unless given, [N, S, 4], S <= 16) n_steps steps of SGD with momentum on the fit loss, the step sizes lr (angle_lr for the
    angle) times gamma after every step; the start whose last recorded loss is smallest wins.  Returns (params [N, 4] = x, y,
    scale, angle; loss [N]) and, with return_all or return_trace, a dict as third value: best [N] int32, all_params [N, S, 4],
    all_loss [N, S] (return_all), trace [N, S, n_steps, 9] = the parameters, the loss and the gradient of every step
    (return_trace).  curve and prototype as in lens_fit_grad.  The loss is the one of the last step before its update, as the
    reference records it; n_steps = 0 evaluates the starts"""
    who = "fit_lens_shapes"
    n_steps, lr, angle_lr, momentum, gamma, weight = _check_schedule(n_steps, lr, angle_lr, momentum, gamma, lens_fit_weight,
                                                                     "lens_fit_weight", who)
    curve, n, k, p, prototype = _fit_args(curve, prototype, who)
    if starts is None:
        starts = lens_fit_starts(curve)
    else:
        starts = _check_dev_tensor(starts, "starts", who, curve.device)
        _check_starts_shape(tuple(starts.shape), n, who)
    return _fit_result(lambda want: _lf_run(curve, k, p, prototype, starts, n_steps, lr, angle_lr, gamma, momentum, weight, want),
                       starts, n_steps, return_all, return_trace)


# ---- the plus shape's fit: loss, gradient and the SGD loop over up to nine starts in one launch (hint_plusfit.hip) ----
#     fit_plus_shape_to_points(points)                                   best_shape_fit.py:93-129, per row at eval_shapes.py:85-87
#     points_to_plus_loss(points, params, corner_weight).backward()      best_shape_fit.py:54-65
#     init_plus_params(angle, xshift, yshift, center)                    best_shape_fit.py:69-79, over the xyshifts of :100
#     fit_line(points)                                                   best_shape_fit.py:83-97: RANSAC, random; here every pair
# One launch of hint_plusfit_run per call: no autograd graph, no per-row host work; the arithmetic, the selected segments and
# corner points, the order of the sums, the clamp-tie rule and the update rule are fixed (include/hint_amd.h).
PLUS_STARTS = ((0.0, 0.0), (-1.5, -1.5), (-1.5, 0.0), (-1.5, 1.5), (0.0, -1.5), (0.0, 1.5), (1.5, -1.5), (1.5, 0.0), (1.5, 1.5))
PLUS_FIT_STEPS = 400
MAX_ANGLE_POINTS = 128     # plus_dominant_angle looks at every pair of points against every point
ANGLE_RESIDUAL = 0.05      # fit_line's residual_threshold


def _check_plus_starts_shape(shape, n_rows: int, who: str) -> int:
    shape = tuple(shape)
    if len(shape) != 3 or shape[0] != n_rows or shape[2] != PLUS_PARAMS or not 1 <= shape[1] <= MAX_STARTS:
        raise HintAmdError(f"{who}: starts must have shape [{n_rows}, S, 9] with S 1..{MAX_STARTS}: xlength, ylength, xwidth, "
                           f"ywidth, xshift, yshift, xoffset, yoffset, angle (got {shape})")
    return shape[1]


def _check_number(v, name: str, who: str) -> float:
    """any number, NaN and the infinities included"""
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise HintAmdError(f"{who}: {name} must be a number (got {type(v).__name__})")
    return float(v)


def _pf_run(curve: torch.Tensor, k: int, p: int, starts: torch.Tensor, n_steps: int = 0, lr: float = 0.1, angle_lr: float = 0.01,
            gamma: float = 1.0, momentum: float = 0.0, corner_weight: float = 1.0, corner_decay: bool = False,
            stop_loss: float = 0.0, want=("params", "loss", "best", "n_run", "all_params", "all_loss", "grad"),
            max_groups: int = 0, out=None):
    """one hint_plusfit_run on checked arguments: a dict of the outputs named in `want` (params [N, 9], loss [N], best [N] int32,
    n_run [N] int32, all_params [N, S, 9], all_loss [N, S], grad [N, S, 9], trace [N, S, n_steps, 19]).  k = 0: curve is
    [N, P, 2] points.  out: tensors to write into instead of new ones (the tests' guarded buffers)"""
    fields = dict(corner_weight=corner_weight, stop_loss=stop_loss, corner_decay=1 if corner_decay else 0)
    return _fit_run(_lib.PlusFitDesc, "hint_plusfit_run", PLUS_PARAMS, fields, curve, k, p, starts, n_steps, lr, angle_lr, gamma,
                    momentum, want, max_groups, out)


def plus_fit_grad(curve: torch.Tensor, params: torch.Tensor, corner_weight: float = 1.0):
    """the reference's points_to_plus_loss(points, params, corner_weight) and its autograd gradient by the nine parameters, for
    every row: (loss [N], grad [N, 9]) fp32 - one launch, no autograd graph.  curve is [N, 4K] coefficients, traced at 100 points
    as the fit's points are, or [N, P, 2] points; params [N, 9], [1, 9] or [9].  Where two segments (or curve points) are equally
    near, the gradient is the one of the first; where a clamp's two arguments are equal, the one of the unclamped side"""
    who = "plus_fit_grad"
    weight = _check_real(corner_weight, "corner_weight", who, nonneg=False)
    if params is None:
        raise HintAmdError(f"{who}: params must be a tensor (got None)")
    curve, n, k, p = _curve_arg(curve, FIT_POINTS, who)
    starts = _plus_params(params, n, who, curve.device).reshape(n, 1, PLUS_PARAMS)
    res = _pf_run(curve, k, p, starts, 0, corner_weight=weight, want=("all_loss", "grad"))
    return res["all_loss"].reshape(n), res["grad"].reshape(n, PLUS_PARAMS)


def _fit_points(curve: torch.Tensor, k: int, p: int) -> torch.Tensor:
    """the curve's points [N, P, 2]: traced from coefficients, or the given ones"""
    return _hd_run(curve, k, p, None, want_points=True)[3] if k else curve


def plus_dominant_angle(curve: torch.Tensor) -> torch.Tensor:
    """[N] fp32: the dominant angle of every row's points, the deterministic stand-in for the reference's fit_line (RANSAC with
    residual_threshold 0.05 over 100 random minimal samples): here every minimal sample is looked at.  Candidates are all pairs
    i < j of points with x_i != x_j; a pair's inliers are the points k with |y_k - line(x_k)| <= 0.05; the winner is the first
    pair in row-major order with the most inliers; angle = atan(the slope of the least-squares line through the winner's inliers).
    curve is [N, 4K] coefficients, traced at 100 points, or [N, P, 2] points with P <= 128 (plain torch on the [P, P, P]
    residuals, at most 2^24 of them at a time).  A row without a candidate, or whose inliers share one x, gets 0; a row that
    holds a value that is not finite gets an unspecified angle; no index comes from it and no other row is touched"""
    who = "plus_dominant_angle"
    curve, n, k, p = _curve_arg(curve, FIT_POINTS, who)
    if p > MAX_ANGLE_POINTS:
        raise HintAmdError(f"{who}: the angle looks at every pair of points against every point and serves at most "
                           f"{MAX_ANGLE_POINTS} points a row (got {p}); pass angle to plus_fit_starts / fit_plus_shapes")
    pts = _fit_points(curve, k, p)
    dev = curve.device
    out = torch.empty(n, dtype=torch.float32, device=dev)
    flat = torch.arange(p * p, device=dev)
    upper = (flat // p) < (flat % p)                                          # i < j
    step = max(1, (1 << 24) // (p * p * p))
    for a in range(0, n, step):
        c = pts[a:a + step]
        m = c.shape[0]
        x, y = c[:, :, 0], c[:, :, 1]
        dx, dy = x[:, None, :] - x[:, :, None], y[:, None, :] - y[:, :, None]             # [m, i, j]: point j - point i
        valid = (upper.reshape(p, p)[None] & (dx != 0)).reshape(m, p * p)
        slope = (dy / dx).reshape(m, p * p)
        icpt = y[:, :, None].expand(m, p, p).reshape(m, p * p) - slope * x[:, :, None].expand(m, p, p).reshape(m, p * p)
        resid = (y[:, None, :] - (slope[:, :, None] * x[:, None, :] + icpt[:, :, None])).abs()          # [m, pair, k]
        cnt = torch.where(valid, (resid <= ANGLE_RESIDUAL).sum(2), -1)
        first = torch.where(cnt == cnt.amax(1, keepdim=True), flat, p * p).amin(1).clamp_(max=p * p - 1)
        rows = torch.arange(m, device=dev)
        inl = ((resid[rows, first] <= ANGLE_RESIDUAL) & valid[rows, first][:, None]).to(torch.float32)   # [m, k]
        cn = _tree_sum(inl)
        xm, ym = _tree_sum(inl * x) / cn, _tree_sum(inl * y) / cn
        sxx, sxy = _tree_sum(inl * (x - xm[:, None]) ** 2), _tree_sum(inl * (x - xm[:, None]) * (y - ym[:, None]))
        out[a:a + step] = torch.where(sxx > 0, torch.atan(sxy / sxx), torch.zeros_like(sxx))
    return out


def _check_angle(angle, n_rows: int, device, who: str) -> torch.Tensor:
    angle = _check_dev_tensor(angle, "angle", who, device)
    if tuple(angle.shape) != (n_rows,):
        raise HintAmdError(f"{who}: angle must have shape [{n_rows}] (got {tuple(angle.shape)})")
    return angle


_PLUS_SHIFTS = {}            # device -> PLUS_STARTS as a [9, 2] tensor there


def _plus_start_shifts(device) -> torch.Tensor:
    """PLUS_STARTS on the device, uploaded once: torch.tensor(list, device=...) copies from pageable host memory, which blocks
    the host until the current stream has run dry - once per device, not once per call"""
    t = _PLUS_SHIFTS.get(device)
    if t is None:
        t = _PLUS_SHIFTS[device] = torch.tensor(PLUS_STARTS, dtype=torch.float32, device=device)
    return t


def plus_fit_starts(curve: torch.Tensor, angle: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N, 9, 9] fp32: the nine starts of the reference's fit_plus_shape_to_points for every row, computed on the device -
    init_plus_params for the nine (xshift, yshift) of its list, in its order: lengths 5, widths 2, the offsets at the mean of the
    curve's points (a traced curve's repeated end point included; the batch-independent sum of lens_fit_starts) and the angle:
    `angle` [N], or plus_dominant_angle(curve).  curve is [N, 4K] coefficients, traced at 100 points, or [N, P, 2] points"""
    who = "plus_fit_starts"
    curve, n, k, p = _curve_arg(curve, FIT_POINTS, who)
    angle = plus_dominant_angle(curve) if angle is None else _check_angle(angle, n, curve.device, who)
    centre = _tree_sum(_fit_points(curve, k, p)) / p
    out = torch.empty(n, len(PLUS_STARTS), PLUS_PARAMS, dtype=torch.float32, device=curve.device)
    out[:, :, 0:2] = 5.0
    out[:, :, 2:4] = 2.0
    out[:, :, 4:6] = _plus_start_shifts(curve.device)[None]
    out[:, :, 6:8] = centre[:, None, :]
    out[:, :, 8] = angle[:, None]
    return out


def fit_plus_shapes(curve: torch.Tensor, *, starts: Optional[torch.Tensor] = None, angle: Optional[torch.Tensor] = None,
                    n_steps: int = PLUS_FIT_STEPS, lr: float = 0.1, angle_lr: float = 0.01, momentum: float = 0.2,
                    gamma: float = 0.1 ** (1 / 400), corner_weight: float = 1.0, corner_decay: bool = True,
                    stop_loss: float = 0.005, return_all: bool = False, return_trace: bool = False):
    """the reference's fit_plus_shape_to_points for every row in one launch: from each of the row's starts in turn
    (plus_fit_starts(curve, angle) unless given, [N, S, 9], S <= 16) n_steps steps of SGD with momentum on the fit loss, the step
    sizes lr (angle_lr for the angle) times gamma after every step, the corner weight corner_weight (1 - i / n_steps) at step i
    (constant without corner_decay); a start whose last recorded loss is below stop_loss ends the row (stop_loss <= 0 or NaN:
    every start runs); the start that ran with the smallest loss wins.  Returns (params [N, 9] = xlength, ylength, xwidth, ywidth,
    xshift, yshift, xoffset, yoffset, angle; loss [N]) and, with return_all or return_trace, a dict as third value: best [N] int32,
    n_run [N] int32 (the starts that ran), all_params [N, S, 9], all_loss [N, S] (return_all; a start that did not run holds
    itself and +inf), trace [N, S, n_steps, 19] = the parameters, the loss and the gradient of every step (return_trace; NaN for
    a start that did not run).  curve as in plus_fit_grad.  The loss is the one of the last step before its update, as the
    reference records it; n_steps = 0 evaluates the starts at corner_weight"""
    who = "fit_plus_shapes"
    n_steps, lr, angle_lr, momentum, gamma, weight = _check_schedule(n_steps, lr, angle_lr, momentum, gamma, corner_weight,
                                                                     "corner_weight", who)
    stop_loss = _check_number(stop_loss, "stop_loss", who)
    if not isinstance(corner_decay, bool):
        raise HintAmdError(f"{who}: corner_decay must be a bool (got {type(corner_decay).__name__})")
    curve, n, k, p = _curve_arg(curve, FIT_POINTS, who)
    if starts is None:
        starts = plus_fit_starts(curve, angle)
    else:
        if angle is not None:
            raise HintAmdError(f"{who}: both starts and angle are given (the angle only makes the default starts)")
        starts = _check_dev_tensor(starts, "starts", who, curve.device)
        _check_plus_starts_shape(tuple(starts.shape), n, who)
    return _fit_result(lambda want: _pf_run(curve, k, p, starts, n_steps, lr, angle_lr, gamma, momentum, weight, corner_decay,
                                            stop_loss, want),
                       starts, n_steps, return_all, return_trace, extra=("n_run",))


# ---- IoU / DICE of a curve and a fitted shape, and the evaluation loop's four columns (hint_overlap.hip) ----
#     iou_and_dice_lens_shape(prototype, params, points)                 best_shape_fit.py:265-271, per row at run_experiments.py:150-159
#     iou_and_dice_plus_shape(params, points)                            best_shape_fit.py:133-139, per row at eval_shapes.py:88-95
# One launch of hint_overlap_run per call: the area of the intersection as a sum over pairs of edges - no clipping, no host loop,
# no host synchronisation; the arithmetic and the order of the sums are fixed (include/hint_amd.h).  A curve that crosses itself
# (crossings > 0) gets the winding-weighted value, where the reference rebuilds the polygon with shapely's buffer(0): send those
# rows, and only those, to shapely if its rule matters.  get_lens_prototype stays on the host; the prototype is the caller's.
MIN_POLYGON_POINTS = 3
Overlap = namedtuple("Overlap", ["iou", "dice", "areas", "crossings"])
ShapeScores = namedtuple("ShapeScores", ["iou", "dice", "max_h", "avg_h", "crossings", "params"])


def _polygon_curve(curve, n_points, who: str):
    curve, n, k, p = _curve_arg(curve, n_points, who)
    if p < MIN_POLYGON_POINTS:
        raise HintAmdError(f"{who}: a closed curve needs {MIN_POLYGON_POINTS}..{MAX_DENSE_POINTS} points (got {p})")
    return curve, n, k, p


def _ov_run(curve: torch.Tensor, k: int, p: int, polygon: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None,
            params: Optional[torch.Tensor] = None, plus_params: Optional[torch.Tensor] = None,
            want=("areas", "iou", "dice", "crossings"), max_groups: int = 0, out=None):
    """one hint_overlap_run on checked arguments: a dict of the outputs named in `want` (areas [N, 3] = area of the template, of
    the curve, of the intersection; iou [N]; dice [N]; crossings [N] int32).  k = 0: curve is [N, P, 2] points.  The template is
    polygon (with offsets, params as in _hd_run) or the outline of plus_params [N, 9]; neither: crossings alone.
    out: tensors to write into instead of new ones (the tests' guarded buffers)"""
    n, dev = curve.shape[0], curve.device
    desc = _lib.OverlapDesc()
    _set_curve(desc, curve, n, k, p)
    desc.a_points = polygon.data_ptr() if polygon is not None else None
    desc.n_template = polygon.shape[0] if polygon is not None else 0
    desc.a_offsets = offsets.data_ptr() if offsets is not None else None
    desc.a_params = params.data_ptr() if params is not None else None
    desc.plus_params = plus_params.data_ptr() if plus_params is not None else None
    res = _outputs(desc, dict(areas=((n, 3), _F32), iou=((n,), _F32), dice=((n,), _F32), crossings=((n,), _I32)), want, out, dev)
    desc.max_groups = max_groups
    _run_desc("hint_overlap_run", desc, dev)
    return res


def _overlap_args(curve, polygon, params, offsets, n_points, who: str):
    curve, n, k, p = _polygon_curve(curve, n_points, who)
    polygon = _check_dev_tensor(polygon, "polygon", who, curve.device)
    t_pts = _check_template_shape(tuple(polygon.shape), offsets is not None, who)
    if t_pts < MIN_POLYGON_POINTS:
        raise HintAmdError(f"{who}: polygon must hold at least {MIN_POLYGON_POINTS} points (got shape {tuple(polygon.shape)})")
    if offsets is not None:
        offsets = _check_offsets(offsets, n, t_pts, who).to(curve.device)
    if params is not None:
        params = _check_dev_tensor(params, "params", who, curve.device)
        _check_params_shape(tuple(params.shape), n, who)
        params = params.reshape(-1, 4).expand(n, 4).contiguous()
    return curve, k, p, polygon, offsets, params


def polygon_overlap(curve: torch.Tensor, polygon: torch.Tensor, params: Optional[torch.Tensor] = None, *, offsets=None,
                    n_points: int = 100) -> Overlap:
    """the overlap of every row's closed curve with a closed polygon: Overlap(iou [N], dice [N], areas [N, 3] = the area of the
    polygon, of the curve and of their intersection, crossings [N] int32 = the proper self-crossings of the curve), fp32.

    curve     [N, 4K] coefficients, traced at n_points here, or [N, P, 2] points, 3 <= P <= 1024 (n_points is then ignored);
              the last point is joined to the first
    polygon   [M, 2] vertices in order, 3 <= M <= 4096, either orientation, shared by all rows; or, with offsets (int64 [N + 1],
              ascending from 0 to T, on the host or the device), [T, 2] of which row n owns polygon[offsets[n]:offsets[n + 1]]
    params    None, or [N, 4] (or [4]) = x, y, scale, angle: the polygon is first moved as lens_points_from_params does

    For simple polygons the intersection is the one shapely computes; a curve with crossings > 0 counts every region by the
    product of the two winding numbers.  A row with a value that is not finite, or with a bad offsets range, gets NaN and -1"""
    who = "polygon_overlap"
    curve, k, p, polygon, offsets, params = _overlap_args(curve, polygon, params, offsets, n_points, who)
    res = _ov_run(curve, k, p, polygon, offsets, params)
    return Overlap(res["iou"], res["dice"], res["areas"], res["crossings"])


def lens_iou_dice(curve: torch.Tensor, prototype: torch.Tensor, params: torch.Tensor):
    """the reference's iou_and_dice_lens_shape(prototype, params, points) for every row: (iou [N], dice [N], crossings [N] int32).
    curve is [N, 4K] coefficients, traced at 100 points as the reference's are, or [N, P, 2] points; prototype [M, 2], the
    outline's vertices in order, 3 <= M <= 4096; params [N, 4], [1, 4] or [4] = x, y, scale, angle.  Where crossings is 0 the
    curve is simple and the values are the reference's; elsewhere see polygon_overlap"""
    who = "lens_iou_dice"
    if params is None:
        raise HintAmdError(f"{who}: params must be a tensor (got None)")
    curve, k, p, prototype, _, params = _overlap_args(curve, prototype, params, None, FIT_POINTS, who)
    res = _ov_run(curve, k, p, prototype, None, params, want=("iou", "dice", "crossings"))
    return res["iou"], res["dice"], res["crossings"]


def plus_iou_dice(curve: torch.Tensor, params: torch.Tensor):
    """the reference's iou_and_dice_plus_shape(params, points) for every row: (iou [N], dice [N], crossings [N] int32).  The
    polygon is the plus shape's outline, placed inside the kernel: the twelve vertices plus_segments(params)[0][:, :, 0] (a
    dropped segment repeats a vertex, which changes no area).  curve as in lens_iou_dice; params [N, 9], [1, 9] or [9]"""
    who = "plus_iou_dice"
    curve, n, k, p = _polygon_curve(curve, FIT_POINTS, who)
    params = _plus_params(params, n, who, curve.device)
    res = _ov_run(curve, k, p, plus_params=params, want=("iou", "dice", "crossings"))
    return res["iou"], res["dice"], res["crossings"]


def _scores_x(x, who: str) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        _check_no_grad(x, "x", who)
    return _check_x(x, who)


def lens_shape_scores(x: torch.Tensor, prototype: torch.Tensor) -> ShapeScores:
    """the body of the reference's lens-shape evaluation loop (run_experiments.py:144-167) for all rows of x [N, 4K]:
    fit_lens_shapes on the curve at 100 points, lens_iou_dice on the same points, hausdorff_distances of the curve at 1000 points
    to the fitted prototype.  ShapeScores(iou, dice, max_h, avg_h, crossings, params [N, 4]), all [N] on x's device; no host
    synchronisation - the means are the caller's to take"""
    who = "lens_shape_scores"
    x = _scores_x(x, who)
    params, _ = fit_lens_shapes(x, prototype)
    iou, dice, crossings = lens_iou_dice(x, prototype, params)
    max_h, avg_h = hausdorff_distances(x, prototype, params, n_points=1000)
    return ShapeScores(iou, dice, max_h, avg_h, crossings, params)


def plus_shape_scores(x: torch.Tensor) -> ShapeScores:
    """the body of the reference's plus-shape evaluation loop (eval_shapes.py:82-103) for all rows of x [N, 4K]: fit_plus_shapes
    on the curve at 100 points, plus_iou_dice on the same points, plus_hausdorff_distances of the curve at 1000 points to the
    fitted outline.  ShapeScores(iou, dice, max_h, avg_h, crossings, params [N, 9]); no host synchronisation"""
    who = "plus_shape_scores"
    x = _scores_x(x, who)
    params, _ = fit_plus_shapes(x)
    iou, dice, crossings = plus_iou_dice(x, params)
    max_h, avg_h = plus_hausdorff_distances(x, params, n_points=1000)
    return ShapeScores(iou, dice, max_h, avg_h, crossings, params)
