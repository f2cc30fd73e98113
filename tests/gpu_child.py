"""GPU cases in child processes: `python -m tests.<module> <case>` under `timeout -k 10`, one child at a time.  The child
imports torch before it loads the library, which an earlier test module of this pytest process may have loaded already.
A child that dies of a signal, aborts, faults or runs out of time fails its test, and no further child of its module is
started."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_stopped = {}   # module: the child that ended abnormally


def run(module, case, timeout=600, env=None):
    """The output of case `case` of tests/<module>.py, which must exit 0 and end with "ok"."""
    if module in _stopped:
        pytest.fail(f"not started: an earlier child ended abnormally ({_stopped[module]})")
    cmd = [sys.executable, "-m", f"tests.{module}", case]
    if shutil.which("timeout"):
        cmd = ["timeout", "-k", "10", str(timeout)] + cmd
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout + 30)
    except subprocess.TimeoutExpired:
        _stopped[module] = f"{case}: timed out"
        pytest.fail(f"case {case} timed out after {timeout} s")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _stopped[module] = f"{case}: exit {r.returncode}"
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), f"case {case}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout
