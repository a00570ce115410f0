"""The NumPy restatement of the reprojection contract, pinned.  tests/reproject_restatement_digests.json holds SHA-256 digests of
out, out_len and motion (NaNs canonicalised as math_expect.canonical_bits does) that the four separate restatements returned before
they were merged into reproject_expect.reproject -- taken with the modules of the commit before the merge, on the inputs the GPU
tests use: the synthetic buffers of each form at 37 x 29 with seed 7 under the three previous cameras, normals on and off, history
on and off, for the static form ids on and off, moved and unmoved tables, the tight thresholds, and the four small frames; and with
a depth tolerance of 1, under which every depth passes and the carried normal decides taps.  What the shared function returns today
is compared with them, so the restatement is checked against what it was and not against itself."""
import hashlib
import json
import os

import pytest

import math_expect
import reproject_expect as rx
import reproject_instances_expect as ix
import reproject_moving_expect as mx
import reproject_quads_expect as qx

NX, NY, SEED = 37, 29, 7
SMALL = [(1, 1), (16, 16), (17, 1), (1, 33)]
TIGHT = dict(alpha_min=0.75, depth_tol=0.0, normal_min=0.9, max_history=4.0)
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reproject_restatement_digests.json")


def _unmoved(form):
    """The tables of each form in which no record differs, by the form's own unmoved_* functions."""
    spheres, prev_spheres, media, time, prev_time = mx.unmoved_tables()
    t = dict(spheres=spheres, prev_spheres=prev_spheres, media=media, time=time, prev_time=prev_time)
    if form in ("instances", "quads"):
        t["instances"], t["prev_instances"], t["media"] = ix.unmoved_instance_tables()
    if form == "quads":
        t["quads"], t["prev_quads"] = qx.unmoved_quad_tables()
    return t


FORMS = {"static": (rx, rx.synthetic), "moving": (mx, mx.synthetic_moving), "instances": (ix, ix.synthetic_instances),
         "quads": (qx, qx.synthetic_quads)}


def cases(form):
    """(name, keyword arguments of the form's reproject()) for every pinned call of one form."""
    module, synthetic = FORMS[form]
    s = synthetic(NX, NY, SEED)
    tables = {"none": {}} if form == "static" else {"moved": s["tables"], "unmoved": _unmoved(form)}
    if form == "quads":                                  # the quad tables alone unmoved, under moved instances and spheres
        tables["unmoved quads"] = dict(s["tables"], quads=tables["unmoved"]["quads"], prev_quads=tables["unmoved"]["prev_quads"])
    for normals in (False, True):
        for ids in ((False, True) if form == "static" else (True,)):
            for history in (False, True):
                kw = rx.select(s["buffers"], normals, ids, history) if form == "static" else module.select(s["buffers"], normals, history)
                for tname, t in tables.items():
                    for cname, prev in s["cams"].items():
                        name = f"{form} {NX}x{NY} normals={normals} ids={ids} history={history} tables={tname} prev={cname}"
                        yield name, dict(kw, cur=s["cur"], prev=prev, **t)
                        if history and cname == "near":
                            yield name + " tight", dict(kw, cur=s["cur"], prev=prev, **t, **TIGHT)
                        if history and normals and cname != "behind":     # (with the depth test passing, the carried normal decides taps)
                            yield name + " any depth", dict(kw, cur=s["cur"], prev=prev, **t, depth_tol=1.0)
    for nx, ny in SMALL:
        s = synthetic(nx, ny, 100 * nx + ny)
        for cname, prev in s["cams"].items():
            yield f"{form} {nx}x{ny} prev={cname}", dict(s["buffers"], cur=s["cur"], prev=prev, **s.get("tables", {}))


def digest(array):
    return hashlib.sha256(math_expect.canonical_bits(array).tobytes()).hexdigest()


def digests(form):
    """{case name: [digest of out, of out_len, of motion]} with the reproject() the form's module exports."""
    reproject = FORMS[form][0].reproject
    return {name: [digest(a) for a in reproject(**kw)] for name, kw in cases(form)}


@pytest.mark.parametrize("form", list(FORMS))
def test_the_shared_restatement_returns_what_the_four_separate_ones_returned(form):
    with open(DIGESTS) as f:
        pinned = json.load(f)[form]
    got = digests(form)
    assert sorted(got) == sorted(pinned), "the pinned cases and the cases of this test differ"
    assert len(got) >= 12 * (3 if form == "static" else 2)
    bad = [f"{name}: {what}" for name in got for what, g, p in zip(("out", "out_len", "motion"), got[name], pinned[name]) if g != p]
    assert not bad, f"{len(bad)} arrays differ from the pinned restatement, first: {bad[:4]}"
