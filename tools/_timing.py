"""What the tools/*_time.py scripts share: the summary of a list of timings and the commit a tree was built from."""
import os
import statistics
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(us):
    q = statistics.quantiles(us, n=4) if len(us) > 1 else [us[0]] * 3
    return {"median_us": statistics.median(us), "q1_us": q[0], "q3_us": q[2], "min_us": min(us), "max_us": max(us), "reps": len(us)}


def commit_of_tree():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"
