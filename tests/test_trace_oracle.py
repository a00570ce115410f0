"""The oracle's trace entry point (orc_trace_rays, OracleScene.trace) pinned on its own, without a GPU: it returns the t the
oracle's render records for the render's rays, and on every finite ray family of the solid scenes its answer passes the
plain float64 brute force of trace_families.f64_check."""
import numpy as np
import pytest

import trace_families as tf

SCENES = ["two_spheres", "degenerate", "bouncing", "book1", "cornell", "cornell_smoke", "final", "checker", "earth", "perlin",
          "quads", "simple_light", "original", "instanced", "fog", "crowd_4096", "crowd_4097", "crowd_2400",
          "crowd_big"]
MEDIA_SCENES = ("cornell_smoke", "final", "original", "fog")
# crowd_big is left out of the float64 check: its boxes stand on the ground sphere and touch each other, so the check's
# bounds leave over 1 % of the volume family undecided there (it has no off-surface or missed hit; the GPU module checks it)
NX, NY, NS = 48, 32, 4
F64_ROWS = 3000          # rays per batch that go through the float64 brute force (it is O(rays x primitives))
F64_ROWS_CROWD = 300     # the same for the sphere crowds (2 400 .. 4 097 spheres)
# Share of a family's rays that the float64 check may leave undecided.  Only the volume family is capped: the others are
# built on features, window ends and range limits, where the bounds of f64_check leave many rays undecided; those families
# are decided bit for bit against the oracle on the GPU (tests/test_trace_edges.py), and here they must still have every
# reported hit on its surface.
UNDECIDED_CAP = {"volume": 0.01}
# far origins (1e3 .. 1e12 x the scene) are outside the missed-hit check: the first-order bounds do not cover them
NO_MISSED_CHECK = {("scale", 2)}


@pytest.fixture(scope="module")
def scene(art, orc):
    cache = {}

    def get(name):
        if name not in cache:
            img, iw, ih = art.default_texture(name)
            hs = art.HostScene(name, NX, NY, img, iw, ih)
            os_ = orc.OracleScene(name, NX, NY, img, iw, ih)
            rays = tf.ray_sample(orc, os_, NX, NY, NS)
            fam = tf.families(hs, rays, lambda b: os_.trace(b.o, b.d, b.tm, b.tmin, b.tmax)[0])
            cache[name] = (hs, os_, rays, fam)
        return cache[name]
    return get


@pytest.mark.parametrize("name", SCENES)
def test_oracle_trace_matches_its_render(scene, name):
    """With the default window, orc_trace_rays gives every ray of an oracle render the t the render recorded, bit for bit;
    a miss has zero records and material -1; every hit's material is one of the scene's."""
    hs, os_, rays, _ = scene(name)
    t, p, n, uv, mat = os_.trace(rays[:, 0:3], rays[:, 3:6], rays[:, 6])
    assert np.array_equal(t.view(np.uint32), rays[:, 7].view(np.uint32))
    miss = t == tf.FLT_MAX
    assert (mat[miss] == -1).all() and (p[miss] == 0).all() and (n[miss] == 0).all() and (uv[miss] == 0).all()
    assert (mat[~miss] >= 0).all()
    # threads change nothing
    t1, p1, _, uv1, mat1 = os_.trace(rays[:, 0:3], rays[:, 3:6], rays[:, 6], threads=1)
    assert np.array_equal(t1.view(np.uint32), t.view(np.uint32)) and np.array_equal(mat1, mat)
    assert np.array_equal(p1.view(np.uint32), p.view(np.uint32)) and np.array_equal(uv1.view(np.uint32), uv.view(np.uint32))


@pytest.mark.parametrize("name", SCENES)
def test_families_are_well_formed(scene, name):
    """Every finite family is finite and of the planned size; the non-finite family carries a non-finite value or a zero
    direction in every ray."""
    hs, _, _, fam = scene(name)
    for f in tf.FINITE_FAMILIES:
        for b in fam[f]:
            assert len(b.o) >= (200 if f == "window" else 1000), (f, len(b.o))   # window: tmax at the hits' t
            assert np.isfinite(b.o).all() and np.isfinite(b.d).all() and np.isfinite(b.tm).all(), f
            assert np.isfinite(b.tmin)
    nf = fam["nonfinite"][0]
    bad = tf.expected_nonfinite_miss(nf)
    zero = (nf.d == 0).all(1)
    assert (bad | zero).all() and zero.sum() > 0 and bad.sum() > 0


@pytest.mark.parametrize("name", [s for s in SCENES if s not in MEDIA_SCENES + ("crowd_big",)])
def test_oracle_agrees_with_float64(art, scene, name):
    """On every finite family of a solid scene (no media) the oracle's closest hit lies on its primitive and no primitive has
    a clear hit in the window before it (trace_families.f64_check states the bounds).  Undecided rays of the volume family
    are at most 1 %."""
    hs, os_, _, fam = scene(name)
    assert hs.desc.n_media == 0
    report = {}
    for f in tf.FINITE_FAMILIES:
        und = tot = 0
        for k, b in enumerate(fam[f]):
            rows = F64_ROWS_CROWD if name.startswith("crowd") else F64_ROWS
            b = tf.Batch(*(x[:rows] if isinstance(x, np.ndarray) else x for x in b))
            t, _, _, _, _ = os_.trace(b.o, b.d, b.tm, b.tmin, b.tmax)
            prim, inst = _oracle_prim(hs, b, t)
            r = tf.f64_check(hs, b, t, prim, inst)
            assert len(r.off_surface) == 0, (f, k, r.off_surface[:5], t[r.off_surface[:5]])
            if (f, k) not in NO_MISSED_CHECK:
                assert len(r.missed) == 0, (f, k, r.missed[:5], t[r.missed[:5]])
            und += int((~b.exact[r.undecided]).sum())
            tot += int((~b.exact).sum())
        report[f] = (und, tot)
        if f in UNDECIDED_CAP:
            assert und <= UNDECIDED_CAP[f] * tot, (f, und, tot)
    print(name, report)


def _oracle_prim(hs, b, t):
    """The oracle reports no primitive: any hit is matched against every primitive (prim = -2 stands for 'any')."""
    prim = np.where(t < tf.FLT_MAX, -2, -1)
    return prim, np.full(len(t), -1)
