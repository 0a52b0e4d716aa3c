"""What the tools/*_time.py scripts share: the HIP-event timing of a call, the warm-up and alternation of a script's routes, the
summary of a list of timings, the commit a tree was built from, and the driver that gives every size a child process."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(us):
    q = statistics.quantiles(us, n=4) if len(us) > 1 else [us[0]] * 3
    return {"median_us": statistics.median(us), "q1_us": q[0], "q3_us": q[2], "min_us": min(us), "max_us": max(us), "reps": len(us)}


def commit_of_tree():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def timed(fn):
    """(microseconds between two HIP events on the current stream around fn(), what fn returned)"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out


def alternate(routes, reps, warmup, after_warmup=None):
    """every route of the dict `warmup` times, then `reps` rounds of each in turn - clocks and caches drift for all routes alike:
    ({name: the microseconds of each round}, {name: the last output}).  after_warmup: called between the two, on an idle device"""
    import torch
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    if after_warmup:
        after_warmup()
    us = {name: [] for name in routes}
    outs = {}
    for _ in range(reps):
        for name, fn in routes.items():
            dt, out = timed(fn)
            us[name].append(dt)
            outs[name] = out
    return us, outs


def parser(out_name, warmup, commit=True):
    """the arguments the per-size scripts share"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name))
    if commit:
        ap.add_argument("--commit", default=None, help="the commit the tree was built from (default: git rev-parse HEAD)")
    ap.add_argument("--one", type=int, default=0, help="(internal) time this N and print its JSON row")
    ap.add_argument("--reps", type=int, default=0, help="(internal) repetitions of --one")
    return ap


def emit_row(row, lib):
    """a child's result, for drive(): the row with the device's name and the library's build string"""
    import torch
    row["device"], row["build"] = torch.cuda.get_device_name(0), lib.hint_build_info().decode()
    print("ROW " + json.dumps(row))
    return 0


def print_stats(n, row, names, width=6, digits=12):
    for name in names:
        s = row[name]
        print(f"N={n} {name:{width}s} median {s['median_us']:{digits}.1f} us  quartiles {s['q1_us']:.1f} .. {s['q3_us']:.1f}  "
              f"range {s['min_us']:.1f} .. {s['max_us']:.1f}  ({s['reps']} repetitions)")


def drive(script, limit_s, sizes, res, out, summary):
    """for each (n, child arguments) of sizes: `script --one n <child arguments>` in a process of its own under limit_s seconds,
    its ROW line into res["shapes"][str(n)] (device and build into res), summary(n, row), and res written to `out` anew.  The
    first size that runs out of time, exits with a status or prints no row ends the run with 1: nothing more is started on the
    device after it"""
    for n, child_args in sizes:
        cmd = [sys.executable, os.path.abspath(script), "--one", str(n)] + [str(a) for a in child_args]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit_s)
        except subprocess.TimeoutExpired:
            print(f"N={n}: no result within {limit_s} s; stopping")
            return 1
        rows = [ln[4:] for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        if p.returncode != 0 or not rows:
            print(f"N={n}: exit status {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            return 1
        row = json.loads(rows[-1])
        res["device"], res["build"] = row.pop("device"), row.pop("build")
        res["shapes"][str(n)] = row
        summary(n, row)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(res, open(out, "w"), indent=1)
    print("wrote", out)
    return 0
