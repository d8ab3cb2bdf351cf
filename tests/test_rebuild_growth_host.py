"""Without a GPU: the growth layouts of tests/rebuild_growth_world.py do outgrow a quarter of slack (the host build counts them), and
rt_sequence parses and refuses its key tree=build|rebuild as it does the other keys, before any device work."""
import os
import re
import subprocess

import pytest

import rebuild_growth_world as gw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dd2360-raytracing_amd", "rt_sequence")


def test_the_grown_layout_exceeds_a_quarter_of_slack(rt):
    """pairs, bucket entries and large spheres of `grown` exceed 1.25 x those of `first` (measured: pairs and entries 2386 -> 6269,
    large spheres 3 -> 669), so a rebuild from `first` to `grown` cannot fit what the handle kept.  The registrations fall (3992 ->
    2660: the enlarged spheres leave the grid for the large list) and so do the leaf buckets (one cell column instead of 64)."""
    W = rt.World(gw.N, gw.NX, gw.NY)
    first, grown = W.spheres, gw.grown_spheres(W.spheres)
    assert len(gw.small_slots(first)) >= gw.N - 4
    a, b = gw.counts(rt, first, W.camera), gw.counts(rt, grown, W.camera)
    print("first %s\ngrown %s" % (a, b))
    for k in ("pairs", "entries", "large"):
        assert b[k] > gw.SLACK * a[k] + 64, (k, a[k], b[k])          # (+ 64: the least slack a rebuild leaves)
    assert a["pairs"] == a["entries"] and b["pairs"] == b["entries"]      # no ghost among the stored spheres, nothing dropped
    assert b["pairs"] <= 16 * gw.N + 65536                          # far below the device build's limit: it must not decline
    W.close()


REFUSED = [(["tree=bogus"], "tree"), (["tree="], "tree"), (["mode=progressive", "tree=rebuild"], "tree"),
           (["tree=rebuild", "frames=0"], "frames"), (["tree=build", "frames=0"], "frames")]


@pytest.mark.parametrize("tokens,key", REFUSED, ids=[" ".join(t) for t, _ in REFUSED])
def test_the_tree_key_is_parsed_and_refused_before_any_device_work(rt, tmp_path, tokens, key):
    """exit code 99 and one line that names the key at fault: a bad value names `tree`; a good one is accepted, and the refusal that
    follows names the other key"""
    p = subprocess.run([EXE] + tokens, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert p.returncode == 99, (p.returncode, p.stderr)
    assert re.match(r"rt_sequence: %s: " % re.escape(key), p.stderr), p.stderr
    assert "rt_device_check" not in p.stderr and "spheres of radius" not in p.stderr and len(p.stderr.splitlines()) == 1
    assert os.listdir(tmp_path) == []
