"""The three host units of libblinkyhip that stand alone - the worker pool (bk_hostpool.cpp), the code cache's trust checks
(bk_codecache.cpp) and the resident apply's planner (bk_resident_plan.cpp) - each linked into a small program of its own
(tests/host/pool_check.cpp, codecache_check.cpp, resplan_check.cpp; built by tests/host/Makefile's `all`).  The programs print what
failed and exit non-zero."""
import os
import subprocess

import pytest

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")


def _run(name, **env_changes):
    exe = os.path.join(HOST, name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST, name])
    env = dict(os.environ)
    env.pop("BLINKY_HIP_FIXUP_THREADS", None)
    env.update(env_changes)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{name} exited with {r.returncode}:\n{r.stdout}{r.stderr}"
    return r.stdout


@pytest.mark.parametrize("threads", [None, "1"])
def test_worker_pool(threads):
    """every index once, a throwing section leaves no worker behind, concurrent submitters - with the machine's pool and with a
    pool of one thread (the variable is read when the pool is first used: a process each)"""
    out = _run("pool_check", **({"BLINKY_HIP_FIXUP_THREADS": threads} if threads else {}))
    if threads:
        assert "pool of 1 threads" in out


def test_code_cache_trust():
    """SHA-256 vectors, sealed-file round trip, and every kind of file or directory that must be a miss"""
    _run("codecache_check")


def test_resident_planner():
    """every plan that fits holds what the resident kernel and its collector rely on, over a seeded sweep of block maps; the stride
    planner refuses a plan with an empty stride group; the form choice takes each rung only when the rungs before it do not fit"""
    assert "resplan_check ok" in _run("resplan_check")
