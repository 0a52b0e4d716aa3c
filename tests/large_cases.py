"""The cases of the large-index tests (tests/test_gpu_large_rows.py and, at the end of this file, tests/test_gpu_large_flow.py;
checked without a GPU by tests/test_large_cases_cpu.py): every descriptor kernel once at the smallest size at which its widest
per-row array holds more than 2^31 elements - so that element indices pass 2^31 and byte offsets pass 2^31 and 2^32 inside one
call - and the rows such a run is probed at.

Three ledgers, and every entry point that takes a descriptor is in exactly one (tests/test_large_cases_cpu.py holds them against
include/hint_amd.h): ROW_CASES, the cases; LIMITED, entry points whose documented limits keep every offset below 2^31, each with
the test that runs it AT that limit; NOT_COVERED, the two left out, with the reason.

A case's N is computed here from the width of the named array (rows_past, then ragged_up): never typed by hand.  `arrays` lists
every device array of the case as (name, elements, bytes per element); `peak` is what the test asks torch.cuda.mem_get_info for
before it allocates anything: the arrays plus 2 GiB for chunked temporaries (no temporary, and no float64 copy, is larger).

Probe rows (probe_rows): the first 64 rows, the last 80 (the ragged tail), a picket of about 400 rows at a prime stride, and the
rows on either side of r* = ceil(2^k / width), k = 29, 30, 31 - where the element index of the widest array crosses 2^29, 2^30
and 2^31, i.e. where its byte offset crosses 2^31 and 2^32 and where a 32-bit element index wraps.
"""
import gc

GIB = 1 << 30
EDGE = 1 << 31                      # elements the named array must exceed
CROSSINGS = (29, 30, 31)
HEAD, TAIL, PICKET = 64, 80, 400
SLACK = 2 * GIB                     # room for chunked temporaries
CAP = 24 * GIB                      # no case may need more
CHUNK_ELEMS = 1 << 28               # elements of a chunked fp32 / int32 temporary (1 GiB; as float64 2 GiB)


def rows_past(width, elems=EDGE):
    """the smallest N with N * width > elems"""
    return elems // width + 1


def ragged_up(n, moduli):
    """the smallest n' >= n + 5 that is a multiple of none of `moduli` (each > 1)"""
    n += 5
    while any(n % m == 0 for m in moduli if m > 1):
        n += 1
    return n


def is_prime(n):
    if n < 2:
        return False
    i = 2
    while i * i <= n:
        if n % i == 0:
            return False
        i += 1
    return True


def picket_stride(N):
    s = max(2, N // PICKET)
    while not is_prime(s):
        s += 1
    return s


def crossing_rows(width):
    """r* for k = 29, 30, 31: the first row that begins at or past element 2^k of an array of `width` elements per row"""
    return [-(-(1 << k) // width) for k in CROSSINGS]


def probe_rows(N, width, extra=(), crossings=None):
    """sorted row numbers: head, tail, picket, two rows on either side of every crossing inside the batch, and `extra`.
    crossings: the rows r* themselves, where the named array is not [N, width] (ragged)"""
    rows = set(range(min(HEAD, N))) | set(range(max(0, N - TAIL), N)) | set(range(0, N, picket_stride(N)))
    for r in crossing_rows(width) if crossings is None else crossings:
        rows |= {q for q in (r - 2, r - 1, r, r + 1) if 0 <= q < N}
    rows |= {int(q) for q in extra if 0 <= q < N}
    return sorted(rows)


def runs_of(rows):
    """[(first, count)] of the maximal runs of consecutive numbers in a sorted list"""
    out = []
    for r in rows:
        if out and out[-1][0] + out[-1][1] == r:
            out[-1][1] += 1
        else:
            out.append([r, 1])
    return [tuple(v) for v in out]


def _case(name, entry, named, width, N, arrays, limit, geometry=None, fixed_n=False, crossings=None, grid=None, **params):
    """grid: (rows a workgroup has in flight, workgroups at most) of an entry point that has no geometry query, from its kernel's
    constants"""
    total = sum(n * b for _, n, b in arrays)
    return dict(name=name, entry=entry, named=named, width=width, N=N, arrays=arrays, bytes=total, peak=total + SLACK,
                limit=limit, geometry=geometry, fixed_n=fixed_n, params=params, grid=grid,
                crossings=crossing_rows(width) if crossings is None else crossings)


def _curve():
    K, P = 25, (2, 3)
    w = 4 * K
    N = ragged_up(rows_past(w), (64, 4, 2048))
    return _case("curve", "hint_curve_run", "x", w, N, [("x", N * w, 4), ("y", N * 2, 4), ("dist", N, 4)], 1 << 30,
                 geometry=("hint_curve_geometry", (N, K, 2)), K=K, P=P)


def _hausdorff_points():
    K, P, M = 5, 128, 3
    w = 2 * P
    N = ragged_up(rows_past(w), (64, 256, 1280))
    return _case("hausdorff_points", "hint_hausdorff_run", "points", w, N,
                 [("x", N * 4 * K, 4), ("params", N * 4, 4), ("points", N * w, 4), ("max_h", N, 4), ("avg_h", N, 4),
                  ("chamfer", 2 * N, 4)], 1 << 30,
                 geometry=("hint_hausdorff_geometry", (N, P, M)), K=K, P=P, M=M)


def ragged_offset(n):
    """a_offsets[n] of the ragged Hausdorff case: row n owns 3 template points, every fifth row (n % 5 == 0) a fourth"""
    return 3 * n + (n + 4) // 5


def ragged_crossing_rows():
    """the rows whose template range is the first to begin at or past element 2^k of a_points [T, 2], k = 29, 30, 31"""
    out = []
    for k in CROSSINGS:
        lo, hi = 0, 1 << 31
        while lo < hi:
            mid = (lo + hi) // 2
            if 2 * ragged_offset(mid) >= 1 << k:
                hi = mid
            else:
                lo = mid + 1
        out.append(lo)
    return out


def _hausdorff_ragged():
    # "about one point a row" would put N at the limit of 2^30 rows, where x and a_offsets alone take 26 GB: three to four points
    # a row is the fewest at which the case stays under the cap
    K, P = 1, 2
    N = ragged_up(ragged_crossing_rows()[-1], (64, 256, 1280))
    T = ragged_offset(N)
    assert T > 1 << 30
    return _case("hausdorff_ragged", "hint_hausdorff_run", "a_points", None, N,
                 [("a_points", 2 * T, 4), ("a_offsets", N + 1, 8), ("x", N * 4 * K, 4), ("max_h", N, 4), ("avg_h", N, 4)],
                 1 << 30, crossings=ragged_crossing_rows(), geometry=("hint_hausdorff_geometry", (N, P, 4)), K=K, P=P, T=T)


def _plus():
    K, P, w = 3, 4, 48                                # segments [N, 12, 2, 2]
    N = ragged_up(rows_past(w), (64, 256, 1280))
    return _case("plus", "hint_plus_run", "segments", w, N,
                 [("segments", N * w, 4), ("params", N * 9, 4), ("x", N * 4 * K, 4), ("counts", N * 12, 4), ("keep", N, 4),
                  ("loss", 2 * N, 4), ("max_h", N, 4), ("avg_h", N, 4)], 1 << 30,
                 geometry=("hint_plus_geometry", (N, P)), K=K, P=P, max_dist=64.0)


def _fit(name, entry, n_par, n_steps, geometry):
    """a fit with its trace [N, S, n_steps, 2 n_par + 1] past 2^31 elements: P = 2 and a small prototype keep a step cheap, S and
    n_steps put N near 1e6"""
    K, P, S = 5, 2, 2
    w = S * n_steps * (2 * n_par + 1)
    N = ragged_up(rows_past(w), (64, 256, 1280))
    arrays = [("trace", N * w, 4), ("x", N * 4 * K, 4), ("starts", N * S * n_par, 4), ("all_params", N * S * n_par, 4),
              ("grad", N * S * n_par, 4), ("all_loss", N * S, 4), ("params", N * n_par, 4), ("loss", N, 4), ("best", N, 4)]
    if name == "plusfit":
        arrays.append(("n_run", N, 4))
    return _case(name, entry, "trace", w, N, arrays, 1 << 30, geometry=(geometry, (N, P)), K=K, P=P, S=S, n_steps=n_steps, M=3,
                 n_par=n_par)


def _overlap():
    # the smallest K, P and M the entry point takes; areas alone: with iou, dice and crossings beside it the case passes the cap.
    # K = 1 makes the curve one point (x[row, 0], x[row, 1]), exactly: its area and the intersection are 0, and the template's
    # area depends on the row through the baseline y0 only
    K, P, M, w = 1, 3, 3, 3                           # areas [N, 3]
    N = ragged_up(rows_past(w), (64, 256, 1280))
    return _case("overlap", "hint_overlap_run", "areas", w, N, [("areas", N * w, 4), ("x", N * 4 * K, 4)], 1 << 30,
                 geometry=("hint_overlap_geometry", (N, P, M)), K=K, P=P, M=M)


def _lensgen():
    w = 64                                            # ring [N, 32, 2]
    N = ragged_up(rows_past(w), (64, 256))
    return _case("lensgen", "hint_lensgen_run", "ring", w, N,
                 [("ring", N * w, 4), ("x", N * 20, 4), ("counts", N, 4), ("eps", 2 * N, 4), ("draws_out", 4 * N, 4)], 1 << 30,
                 seed=0x5EED0123456789AB, offset=(1 << 32) - N // 2)


# hint_plusgen.hip: 16 lanes a row, so PG_WAVE_ROWS rows a wavefront, PG_WAVES wavefronts a workgroup, PG_MAX_WG workgroups at
# most (tests/test_large_cases_cpu.py reads the three from the kernel's text)
PG_WAVE_ROWS, PG_WAVES, PG_MAX_WG = 4, 4, 2048
PG_MODULI = (64, PG_WAVE_ROWS, PG_WAVE_ROWS * PG_WAVES, PG_MAX_WG)


def _plusgen(named):
    """the plus-shape sampler's two wide arrays leave by different code - outline [N, 128, 2] per lane at row * PG_PTS, x [N, 100]
    through LDS as 16-byte pieces at tile * (PG_WAVE_ROWS * PG_ROW / 4) - and each passes 2^31 elements at its own N: a case
    each at the smallest such N, the other array NULL"""
    w = dict(outline=256, x=100)[named]
    N = ragged_up(rows_past(w), PG_MODULI)
    arrays = [(named, N * w, 4), ("y", N * 4, 4)]
    if named == "outline":
        arrays += [("counts", N, 4), ("corners", N, 4)]
    arrays.append(("draws_out", N * 9, 4))
    return _case("plusgen_" + named, "hint_plusgen_run", named, w, N, arrays, 1 << 30, grid=(PG_WAVE_ROWS * PG_WAVES, PG_MAX_WG),
                 seed=0x5EED0123456789AB, offset=(1 << 32) - N // 2)


# hint_epoch.hip: EP_TILE rows a workgroup (gather, standardize), EP_MAX_WG workgroups at most, EP_MAX_SLABS slabs of the moments
EP_TILE, EP_MAX_WG, EP_MAX_SLABS = 256, 2048, 1024


def _epoch():
    """one table x [N, 100] past 2^31 elements and one output of its shape: a whole shuffled epoch gathered (count = N: the
    output's element offsets pass 2^31 as the source's do), the moments over all rows (the slab cap: slab_rows far above 256),
    the standardisation out of place (the tile loop's later trips)"""
    d = 100
    N = ragged_up(rows_past(d), (64, EP_TILE, EP_MAX_WG, EP_MAX_SLABS))
    return _case("epoch", "hint_epoch_run", "out_x", d, N, [("x", N * d, 4), ("out_x", N * d, 4), ("indices_out", N, 8)], 1 << 40,
                 grid=(EP_TILE, EP_MAX_WG), d=d, seed=0xC0FFEE1234567, epoch=3)


def _fcoef():
    p_max, K = 1024, 5
    w = 2 * p_max
    N = ragged_up(rows_past(w), (64, 256))
    assert N >= (1 << 20)
    return _case("fcoef", "hint_fcoef_run", "points", w, N, [("points", N * w, 4), ("counts", N, 4), ("x", N * 4 * K, 4)], 1 << 24,
                 p_max=p_max, K=K)


def _abc():
    ny, N, k = 3, 1 << 30, 64                         # the documented maximum: N is the issue's, not ragged
    return _case("abc", "hint_abc_run", "y", ny, N, [("y", N * ny, 4), ("x", N, 4)], 1 << 30,
                 geometry=("hint_abc_geometry", (N, ny)), fixed_n=True, ny=ny, k=k)


def _corr():
    d = 512
    N = ragged_up(rows_past(d), (64, 256))
    return _case("corr", "hint_corr_run", "x", d, N, [("x", N * d, 4), ("corr", d * d, 8), ("target", d * d, 8)], 1 << 24, d=d)


ROW_CASES = {c["name"]: c for c in (_curve(), _hausdorff_points(), _hausdorff_ragged(), _plus(), _overlap(),
                                       _fit("lensfit", "hint_lensfit_run", 4, 128, "hint_lensfit_geometry"),
                                       _fit("plusfit", "hint_plusfit_run", 9, 64, "hint_plusfit_geometry"), _lensgen(), _fcoef(),
                                       _abc(), _corr(), _plusgen("outline"), _plusgen("x"), _epoch())}

# entry points the large-index tests do not reach, each with the reason (DESIGN.md says the same)
NOT_COVERED = {
    "hint_mmd_run": "its smallest case past 2^31 elements is n ~ 2^19 at d = 4096: about 1e15 MFMA flops for the xx triangle alone",
    "hint_adam_*": "no model of this family comes within two orders of magnitude of 2^31 parameters; the case needs 34 GB",
}

# hint_householder.hip: the limits, and the apply grid - tiles of HH_T rows, HH_APPLY_WAVES wavefronts (a tile each) a workgroup,
# HH_MAX_GRID workgroups at most: a workgroup's tile loop makes a second trip past HH_TRIP rows
HH_GRAD, HH_MAX_B, HH_MAX_D, HH_MAX_N = 2, 1 << 22, 128, 256
HH_T, HH_APPLY_WAVES, HH_MAX_GRID = 16, 4, 1024
HH_TRIP = HH_T * HH_APPLY_WAVES * HH_MAX_GRID

# entry points whose documented limits keep every element offset below 2^31, so that no case past 2^31 elements exists: each with
# the reason, the size query and its arguments AT the limit (`at`), the arguments one past a limit that the query must refuse
# (`over`), the elements of the widest array of a run at the limit (`elements`), and the test that runs the entry point there
LIMITED = {
    "hint_householder_run": dict(
        reason="B <= 2^22 rows of d <= 128 floats: the widest array, [B, d], ends at element 2^29",
        sizer="hint_householder_workspace_bytes", at=(HH_GRAD, HH_MAX_B, HH_MAX_D, HH_MAX_D),
        over=((HH_GRAD, HH_MAX_B + 1, HH_MAX_D, HH_MAX_D), (HH_GRAD, HH_MAX_B, HH_MAX_D + 1, HH_MAX_D),
              (HH_GRAD, HH_MAX_B, HH_MAX_D, HH_MAX_N + 1)),
        elements=HH_MAX_B * HH_MAX_D, test="tests/test_gpu_householder.py::test_the_row_limit"),
}


def abc_plant_rows(case):
    """the k rows the abc case plants its near rows at: first, last, both sides of every crossing, the rest from the picket"""
    N, k = case["N"], case["params"]["k"]
    rows = [0, N - 1]
    for r in crossing_rows(case["width"]):
        rows += [r - 1, r]
    step = picket_stride(N)
    q = step
    while len(rows) < k:
        if q not in rows:
            rows.append(q)
        q += 7 * step
    assert len(set(rows)) == k and all(0 <= r < N for r in rows)
    return rows


# ---- device helpers (torch is imported by the callers that have a GPU) ----
def require_memory(case):
    """skip, naming the figure, when the device has less free memory than the case declares"""
    import pytest
    import torch
    torch.cuda.empty_cache()                          # what earlier tests left in the allocator's cache counts as free
    free, _ = torch.cuda.mem_get_info()
    if free < case["peak"]:
        pytest.skip(f"{case['name']}: needs {case['peak'] / GIB:.1f} GiB of device memory, {free / GIB:.1f} GiB are free")


def release(bufs):
    """drop every buffer of a case and hand the memory back"""
    import torch
    bufs.clear()
    gc.collect()
    torch.cuda.empty_cache()


def fill_chunked(t, make, chunk_elems=CHUNK_ELEMS):
    """t[a:b] = make(b - a) over row chunks of at most chunk_elems elements"""
    per_row = max(1, t[0].numel())
    step = max(1, chunk_elems // per_row)
    for a in range(0, t.shape[0], step):
        b = min(t.shape[0], a + step)
        t[a:b] = make(b - a)
    return t


def count_words(words, value, chunk=CHUNK_ELEMS):
    """how many 4-byte words of a flat int32 view equal `value`, counted in chunks"""
    n = 0
    for a in range(0, words.numel(), chunk):
        n += int((words[a:a + chunk] == value).sum())
    return n


def sum64_chunked(t, chunk=CHUNK_ELEMS):
    """float64 sum of a flat fp32 tensor, in chunks (no float64 copy above 2 GiB)"""
    s = 0.0
    for a in range(0, t.numel(), chunk):
        s += float(t[a:a + chunk].double().sum())
    return s


# ---- the flow kernels (tests/test_gpu_large_flow.py): one case per row-kernel family, on that family's tree of the ledger ----
# family -> the ledger case (tests/instance_cases.py) whose tree, scale and kink cap it takes.  Every family runs as ONE block
# through hint_block_*: a block's tape and workspace are 8 GB and about 7.5 GB at the B where the tape passes 2^31 floats, so the
# two tapes and workspaces of the wave-local chain of 2 (32 GB) do not fit under the cap.
FLOW_CASES = {"wave_local": "wl_pairs_nw8_chain_multi", "general_n3": "n3_alt4_cond_block_multi", "subtree": "subtree_block_multi",
              "lean_fly": "fly_block_multi"}
ROW_TILE = 16                       # hint_dev.h ROWS: batch rows per row tile
TAPE_SLACK = 64                     # hint_host.hpp WS_SLACK: floats behind every [Bp][W] array


def ledger_case(family):
    import instance_cases as ic
    return [c for c in ic.CASES if c.name == FLOW_CASES[family]][0]


def tape_sections(L, d, WT, lean, B):
    """[(first float, floats per row)] of the per-row arrays of a block's tape, by the layout comment of hint_abi.cpp:
    [lane tiles: L x B x d][s: L x B x d][pad to 4][a1: Bp x WT + slack][a2: same][sign bytes]; lean plans keep no a1"""
    act = (2 * L * B * d + 3) // 4 * 4
    Bp = -(-B // ROW_TILE) * ROW_TILE
    return [(l * B * d, d) for l in range(2 * L)] + [(act + i * (Bp * WT + TAPE_SLACK), WT) for i in range(1 if lean else 2)]


def tape_floats_predicted(L, d, WT, lean, B):
    Bp = -(-B // ROW_TILE) * ROW_TILE
    last, _ = tape_sections(L, d, WT, lean, B)[-1]
    return last + Bp * WT + TAPE_SLACK + 2 * (Bp // ROW_TILE * (WT // 16) * 64) // 4


def flow_batch(tape_floats, nr):
    """the smallest B whose tape holds more than 2^31 floats (bisection on tape_floats(B), which never decreases), rounded up to
    the row tile of 16 nr rows, plus 5"""
    lo, hi = 1, 1 << 26
    assert tape_floats(hi) > EDGE
    while lo < hi:
        mid = (lo + hi) // 2
        if tape_floats(mid) > EDGE:
            hi = mid
        else:
            lo = mid + 1
    tile = ROW_TILE * nr
    return -(-lo // tile) * tile + 5, lo


def flow_crossings(sections, B):
    """the rows at which the float index of a tape section crosses 2^29, 2^30 or 2^31: {k: row}"""
    out = {}
    for base, width in sections:
        for k in CROSSINGS:
            r = -(-((1 << k) - base) // width)
            if 0 < r < B and base < (1 << k):
                out.setdefault(k, r)
    return out
