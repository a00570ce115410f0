"""Hand-written scene descriptions in which equal t and exact boundaries decide the pixel.

Every scene is seen through a one-ray camera: horizontal = vertical = 0, no lens, no shutter, so camera_get_ray gives every
sample of every pixel the primary ray o = origin, d = lower_left_corner - origin, both exact; pixels differ only by their seed.
The usual ray is o = (-2, -4, 8), d = (1, 2, -4): three non-zero components (a zero component sends the tier kernel's wave to the
reference walk, away from its reduction), and it reaches the origin at t = 2.  Every t a scene's design rests on is a small
integer or dyadic number the float arithmetic of sphere::hit and quad::hit gives exactly:

  * an axis-aligned quad in the plane z = 0: denom = -4, t = (0 - 8) / -4 = 2, P = (0, 0, 0), alpha and beta dyadic;
  * a sphere through the origin with an integer centre c and radius (|c| = r, c.d > 0): b, c and the discriminant are
    integers, the discriminant a perfect square, and the near root is 2.  (0, 0, -3) r 3: b = -54, disc = 144, t = 42 / 21.

Coincident primitives and primitives through the same point tie there; which of them the frame shows is the rule under test
(tests/oracle_mutants.py lists the rules).  The candidates are Lambertian under solid textures of distinct colours, above a
ground sphere and under a gradient sky, so the winner's colour tints every pixel and the pixels still differ in cost (the
schedule tests need pixels dearer than the mean).  Far filler spheres put the candidates at chosen leaf ordinals: 63 and 64
straddle the tier kernel's slot boundary.  The tree splits the leaf list at the median unless a scene says where.

EDGES is the list; each entry carries the scene, its ray, the candidates of its designed tie (each also as a scene of its own,
for the bit-equality of their t), the expected winner and the mutants it is built to kill.  tests/test_edge_scenes_host.py holds
the conditions on this module from the oracle alone; tests/test_edge_scenes.py renders it on the kernels.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import accelerated_ray_tracer_amd as art
import scene_gen as sg

O, D = (-2.0, -4.0, 8.0), (1.0, 2.0, -4.0)            # reaches the origin at t = 2
NX, NY, NS = 16, 16, 8                                # the host module's frame
PAD = 66                                              # leaves of a padded scene: ordinals 63 and 64 exist, and one slot more than one
# the leaf count of test_kernel_matrix_host.BIG's general family: leaf arrays fit the tier kernel's room, the records do not
BIG_LEAVES, BIG_LEAVES_LEAN = 1500, 2600               # (the lean spheres-only families have more room: BIG's other count)
PALETTE = [(0.9, 0.1, 0.1), (0.1, 0.9, 0.1), (0.1, 0.1, 0.9), (0.9, 0.9, 0.1), (0.9, 0.1, 0.9), (0.1, 0.9, 0.9), (0.9, 0.5, 0.1),
           (0.5, 0.1, 0.9), (0.3, 0.3, 0.3), (0.9, 0.9, 0.9), (0.5, 0.9, 0.3), (0.2, 0.6, 0.9)]


def ray_direction(o, d):
    """What camera_get_ray makes of one_ray_camera(o, d): (o + d) - o in float32.  d itself wherever o + d is exact."""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    return (o + d) - o


def one_ray_camera(o, d):
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    c = art.RtCamera()
    c.origin[:] = o
    c.lower_left_corner[:] = o + d
    c.horizontal[:] = (0, 0, 0)
    c.vertical[:] = (0, 0, 0)
    c.u[:] = (1, 0, 0)
    c.v[:] = (0, 1, 0)
    c.lens_radius, c.time0, c.time1 = 0.0, 0.0, 0.0
    return c


class Builder(sg.Builder):
    def __init__(self, root_split=None):
        super().__init__(np.random.default_rng(0))
        self.root_split = root_split

    def _tree(self, a, b, out):
        """Leaves [a, b) in list order, split at the median; the root where the scene says."""
        i = len(out)
        out.append(None)
        if b - a == 1:
            r, lo, hi = self.leaves[a]
        else:
            mid = (a + b) // 2
            if a == 0 and b == len(self.leaves) and self.root_split is not None:
                mid = self.root_split
            lo1, hi1 = self._tree(a, mid, out)
            lo2, hi2 = self._tree(mid, b, out)
            r, lo, hi = -1, np.minimum(lo1, lo2), np.maximum(hi1, hi2)
        out[i] = (lo, len(out), hi, r)
        return lo, hi

    def paint(self, k):
        return self._mat(sg.LAMBERTIAN, self.t_solid(PALETTE[k % len(PALETTE)]))

    def glass(self, k, ior=1.5):
        return self._mat(sg.DIELECTRIC, ior=ior)

    def mirror(self, k, fuzz=0.0):
        return self._mat(sg.METAL, fuzz=fuzz, albedo=PALETTE[k % len(PALETTE)])

    def glow(self, k, tex=-1):
        return self._mat(sg.LIGHT, tex, albedo=tuple(4.0 * x for x in PALETTE[k % len(PALETTE)]))


# ---------------------------------------------------------------------------------------------------------------- parts
# a part: make(b, k) -> (object, the material(s) it made); k numbers its colour
def sphere(c, r, mat="paint", **kw):
    def make(b, k):
        m = getattr(b, mat)(k, **kw)
        return b.sphere(c, r, m), m
    return make


def quad(Q, u, v, mat="paint", **kw):
    def make(b, k):
        m = getattr(b, mat)(k, **kw)
        return b.quad(Q, u, v, m), m
    return make


def box(lo, hi, order=(0, 1, 2, 3, 4, 5)):
    """Six colours, face f (make_box numbering) in colour k + f."""
    def make(b, k):
        mats = [b.paint(k + f) for f in range(6)]
        return b.box(lo, hi, mats, order), mats
    return make


def moved(part, flags, deg=0.0, offset=(0, 0, 0)):
    def make(b, k):
        child, m = part(b, k)
        return b.instance(child, flags, deg, offset), m
    return make


def fog(part, density):
    """A medium bounded by `part` (whose own material is never seen)."""
    def make(b, k):
        boundary, _ = part(b, k)
        m = b._mat(sg.ISOTROPIC, b.t_solid(PALETTE[k % len(PALETTE)]))
        return b.medium(boundary, density, m), m
    return make


Z0 = quad((-2, -2, 0), (4, 0, 0), (0, 4, 0))           # the plane z = 0 around the origin: t = 2, alpha = beta = 1/2
BALL = sphere((0, 0, -3), 3.0)                         # through the origin: t = 2
BALL2 = sphere((1, 2, -2), 3.0)                        # another one: b = -55, c = 136, disc = 169, t = (55 - 13) / 21 = 2
SLAB = box((-2, -2, -3), (2, 2, 0))                    # its face 0 lies in z = 0: t = 2


def compose(name, parts, ray=(O, D), pad=0, root_split=None, nx=NX, ny=NY, ns=NS, ground=True):
    """parts: [(leaf ordinal, part)].  Every other ordinal below max(pad, last + 1) is a far filler sphere; the ground comes last."""
    b = Builder(root_split)
    at = dict(parts)
    assert len(at) == len(parts)
    n = max(pad, max(at) + 1)
    grey = b.paint(8)
    mats = {}
    for k in range(n):
        if k in at:
            obj, m = at[k](b, len(mats))
            mats[k] = m
            b.leaf(obj)
        else:
            b.leaf(b.sphere((100.0 + 3.0 * (k % 64), 40.0 + 3.0 * (k // 64), -50.0), 1.0, grey))
    if ground:
        b.leaf(b.sphere((0, -1000, 0), 990.0, b.paint(9)))
    g = b.finish(name, one_ray_camera(*ray), nx, ny, ns=ns, background=(0.3, 0.35, 0.5), gradient=1)
    g.part_mats = mats
    return g


def solo(part, ray=(O, D)):
    return compose("solo", [(0, part)], ray, ground=False)


def edge(name, parts, winner, t=2.0, rules=(), ray=(O, D), tied=None, exact=True, seed_base=1984, **kw):
    """winner: leaf ordinal of the expected winner, or (ordinal, face) for a box; None: the primary ray hits nothing.
    tied: the ordinals whose t must be bit-equal (default: all parts).  exact: the camera's ray is (o, d) itself.
    seed_base: the frame's seed (pixel k of a frame draws from the chain seeded seed_base + k)."""
    assert not exact or np.array_equal(ray_direction(*ray), np.asarray(ray[1], np.float32)), "the ray's direction is not exact"
    g = compose(name, parts, ray, **kw)
    at = dict(parts)
    tied = list(at) if tied is None else tied
    if winner is None:
        mat = -1
    elif isinstance(winner, tuple):
        mat = g.part_mats[winner[0]][winner[1]]
    else:
        mat = g.part_mats[winner]
    return SimpleNamespace(name=name, scene=g, o=np.asarray(ray[0], np.float32), d=ray_direction(*ray), winner_mat=mat, seed_base=seed_base,
                           t=None if t is None else np.float32(t), solos=[solo(at[k], ray) for k in tied], rules=set(rules),
                           build=lambda nx, ny, ns, **more: compose(name, parts, ray, nx=nx, ny=ny, ns=ns, **dict(kw, **more)))


# ---------------------------------------------------------------------------------------------------------------- the scenes
def _ties():
    S, Q = BALL, Z0
    far = sphere((0, 0, -20), 4.0)                      # behind everything on the ray: seen only if every candidate is lost
    out = [
        # two and three coincident spheres: the first wins (sphere::hit's t < limit; bvh_hit's strict <)
        edge("spheres/siblings", [(0, S), (1, S), (2, far)], 0, rules=["sphere_tmax_lax"], tied=[0, 1]),
        edge("spheres/apart", [(1, S), (5, S), (7, far)], 1, rules=["sphere_tmax_lax"], pad=8, tied=[1, 5]),
        edge("spheres/63-64", [(63, S), (64, S)], 63, rules=["sphere_tmax_lax"], pad=PAD),
        edge("spheres/triple", [(10, S), (63, S), (64, S)], 10, rules=["sphere_tmax_lax"], pad=PAD),
        # ordinals 0 and 64: one lane of the tier wave meets both, in two slots (its own merge, before the wave's reduction)
        edge("spheres/0-64", [(0, S), (64, S)], 0, rules=["sphere_tmax_lax"], pad=PAD),
        edge("spheres/two-through-a-point", [(0, S), (1, BALL2)], 0, rules=["sphere_tmax_lax"]),
        # (swapped, the second sphere is never asked: its box ends in z = 0, where the ray's interval [.., 2] ends too, and the slab
        # test's `tmax <= tmin` rejects a box met in a single point)
        edge("spheres/two-through-a-point/swapped", [(0, BALL2), (1, S)], 0, rules=["slab_tie_lax"]),
        # coincident quads: the last wins (quad::hit's t <= limit, then bvh_hit's strict <)
        edge("quads/siblings", [(0, Q), (1, Q), (2, far)], 1, rules=["quad_tmax_strict", "bvh_left_lax"], tied=[0, 1]),
        edge("quads/apart", [(1, Q), (5, Q), (7, far)], 5, rules=["quad_tmax_strict", "bvh_left_lax"], pad=8, tied=[1, 5]),
        edge("quads/63-64", [(63, Q), (64, Q)], 64, rules=["quad_tmax_strict", "bvh_left_lax"], pad=PAD),
        edge("quads/triple", [(5, Q), (63, Q), (64, Q)], 64, rules=["quad_tmax_strict", "bvh_left_lax"], pad=PAD),
        edge("quads/triple/root-split-64", [(5, Q), (63, Q), (64, Q)], 64, rules=["quad_tmax_strict", "bvh_left_lax"], pad=PAD, root_split=64),
        # mixed: a quad-type candidate wins over a sphere wherever it stands; among quads the last
        edge("mixed/sphere-quad", [(0, S), (1, Q)], 1, rules=["quad_tmax_strict", "bvh_left_lax"]),
        edge("mixed/quad-sphere", [(0, Q), (1, S)], 0, rules=["slab_tie_lax"]),           # (the sphere's box is met in one point, as above)
        edge("mixed/quad-sphere/box-reaches-further", [(0, Q), (1, BALL2)], 0, rules=["sphere_tmax_lax"]),
        edge("mixed/quad-sphere/63-64", [(63, Q), (64, BALL2)], 63, rules=["sphere_tmax_lax"], pad=PAD),
        edge("mixed/sphere-quad-sphere", [(3, S), (63, Q), (64, S)], 63, rules=["sphere_tmax_lax", "quad_tmax_strict"], pad=PAD),
        edge("mixed/quad-sphere-quad", [(3, Q), (63, S), (64, Q)], 64, rules=["quad_tmax_strict"], pad=PAD),
        # a quad and a box face; the face through translate, and through a rotation by 0 (cos = 1, sin = 0 exactly)
        edge("box/quad-then-face", [(0, Q), (1, SLAB)], (1, 0), rules=["quad_tmax_strict"]),
        edge("box/face-then-quad", [(0, SLAB), (1, Q)], 1, rules=["quad_tmax_strict"]),
        edge("box/63-64", [(63, SLAB), (64, Q)], 64, rules=["quad_tmax_strict"], pad=PAD),
        edge("instance/quad-then-translated-face", [(0, Q), (1, moved(box((6, -2, -3), (10, 2, 0)), sg.TRANSLATE, 0.0, (-8, 0, 0)))], (1, 0),
             rules=["quad_tmax_strict"]),
        edge("instance/translated-face-then-quad", [(0, moved(box((6, -2, -3), (10, 2, 0)), sg.TRANSLATE, 0.0, (-8, 0, 0))), (1, Q)], 1,
             rules=["quad_tmax_strict"]),
        edge("instance/sphere-then-translated-sphere", [(0, S), (1, moved(sphere((8, 0, -3), 3.0), sg.TRANSLATE, 0.0, (-8, 0, 0)))], 0,
             rules=["sphere_tmax_lax", "translate_drops_limit"]),
        edge("instance/quad-then-rotated-face", [(0, Q), (1, moved(SLAB, sg.ROTATE_Y, 0.0))], (1, 0), rules=["quad_tmax_strict"]),
        edge("instance/sphere-then-rotated-sphere", [(0, S), (1, moved(S, sg.ROTATE_Y, 0.0))], 0, rules=["sphere_tmax_lax", "roty_drops_limit"]),
        edge("instance/rotated-translated-63-64", [(63, moved(S, sg.ROTATE_Y | sg.TRANSLATE, 0.0, (0, 0, 0))), (64, moved(SLAB, sg.ROTATE_Y | sg.TRANSLATE, 0.0))],
             (64, 0), rules=["quad_tmax_strict"], pad=PAD),
    ]
    return out


def _boxes():
    """The ray moves towards +x, +y and -z.  A box whose low x (face 3), low y (face 5) and high z (face 0) planes pass through
    the origin is met in an edge or a corner: all those faces at t = 2, and the scan keeps the last of them."""
    behind = sphere((0, 0, -20), 4.0)
    edge_box = box((0, -2, -3), (3, 2, 0))                       # faces 0 and 3 at t = 2: face 3 wins
    corner_box = box((0, 0, -3), (3, 3, 0))                      # faces 0, 3 and 5: face 5 wins
    return [
        edge("box/edge", [(0, edge_box), (1, behind)], (0, 3), rules=["box6_reversed"], tied=[0]),
        edge("box/corner", [(0, corner_box), (1, behind)], (0, 5), rules=["box6_reversed", "quad_edge_lo_out"], tied=[0]),
        edge("box/corner/faces-reordered", [(0, box((0, 0, -3), (3, 3, 0), (5, 3, 1, 0, 2, 4))), (1, behind)], (0, 0), rules=["box6_reversed"], tied=[0]),
        edge("box/corner/63", [(63, corner_box), (64, behind)], (63, 5), rules=["box6_reversed"], pad=PAD, tied=[63]),
        # two boxes sharing the face x = 0, their front faces in z = 0: four faces at t = 2, the second box's low-x face last
        edge("box/shared-face", [(0, box((-3, -2, -3), (0, 2, 0))), (1, box((0, -2, -3), (3, 2, 0))), (2, behind)], (1, 3),
             rules=["box6_reversed", "quad_tmax_strict", "quad_edge_hi_out"], tied=[0, 1]),
        edge("box/shared-face/swapped", [(0, box((0, -2, -3), (3, 2, 0))), (1, box((-3, -2, -3), (0, 2, 0))), (2, behind)], (1, 1),
             rules=["box6_reversed", "quad_tmax_strict"], tied=[0, 1]),
    ]


def _quad_edges():
    """alpha or beta exactly 0 and exactly 1, and two corners; a second quad behind, at t = 3, shows through a lost edge."""
    behind = quad((-7, -8, -4), (16, 0, 0), (0, 16, 0))
    cases = {"alpha-0": (0, -2), "alpha-1": (-4, -2), "beta-0": (-2, 0), "beta-1": (-2, -4), "corner-00": (0, 0), "corner-11": (-4, -4)}
    out = []
    for tag, (qx, qy) in cases.items():
        rules = ["quad_edge_lo_out"] if tag.endswith(("0", "00")) else ["quad_edge_hi_out"]
        out.append(edge(f"quad-edge/{tag}", [(0, quad((qx, qy, 0), (4, 0, 0), (0, 4, 0))), (1, behind)], 0, rules=rules, tied=[0]))
    return out


def _grazing():
    tiny = np.float32(1e-8)
    out = [_tangent()]
    # a ray in the plane of a quad (denom == 0, t = 0 / 0): the guard is what rejects it
    in_plane = ((-2.0, -4.0, 0.0), (1.0, 2.0, 0.0))
    out.append(edge("grazing/in-plane", [(0, quad((-2, -2, 0), (4, 0, 0), (0, 4, 0))), (1, sphere((8, 16, 0), 2.0))], 1, t=None,
                    rules=["quad_denom_unguarded"], ray=in_plane, tied=[]))
    # |denom| exactly 1e-8f (n = (0, 0, 1), d.z = -1e-8f, o.z = 2e-8f: t = 2): a hit; the next float below: parallel
    at = ((-2.0, -4.0, float(np.float32(2) * tiny)), (1.0, 2.0, float(-tiny)))
    under = np.nextafter(tiny, np.float32(0))
    below = ((-2.0, -4.0, float(np.float32(2) * under)), (1.0, 2.0, float(-under)))
    far = sphere((8, 16, 0), 2.0)                               # on both rays' way, far behind the quad
    out.append(edge("grazing/denom-1e-8", [(0, Z0), (1, far)], 0, rules=["quad_denom_lax"], ray=at, tied=[0]))
    out.append(edge("grazing/denom-below-1e-8", [(0, Z0), (1, far)], 1, t=None, rules=[], ray=below, tied=[]))
    # t == tmin = 0.001f exactly.  A quad in the plane z = 0.001f seen from z = 0 along d.z = 1: t = 0.001f / 1, accepted.
    tmin = float(np.float32(0.001))
    out.append(edge("grazing/quad-at-tmin", [(0, quad((-4, -6, tmin), (4, 0, 0), (0, 4, 0)))], 0, t=tmin, rules=["quad_tmin_lax"],
                    ray=((-2.0, -4.0, 0.0), (1.0, 2.0, 1.0)), tied=[0]))
    # A sphere of radius 0.001f around the ray's own origin, d a unit axis: b = 0, disc = r * r, the far root is sqrt(r * r) = r:
    # rejected (t > tmin is strict), and the ray goes on to the sphere behind
    out.append(edge("grazing/sphere-at-tmin", [(0, sphere((-2, -4, 8), tmin)), (1, sphere((-2, -4, -3), 3.0))], 1, t=8.0, rules=["sphere_tmin_lax"],
                    ray=(O, (0.0, 0.0, -1.0)), tied=[], ground=False))
    out += _perpendicular_normal()
    return out


def _perpendicular_normal():
    """A hit whose normal is exactly perpendicular to the ray, past the quad's |denom| guard: a quad with the unit normal
    (a, a, 3e-8), a = 0.70710677, under a rotation by 90 degrees, met by the world ray d = (1, 2, 2).  In the child's frame the ray is
    (-2, 2, 1) and denom = fl(3e-8 * 1 + fl(-2a + 2a)) = 3e-8: not parallel.  In the world the normal is (-/+3e-8, -/+a, +/-a) and
    dot(n, d) = fl(2a + fl(-3e-8 - 2a)) = fl(2a - 2a) = 0: 3e-8 is less than half an ulp of 2a.  rotate_y's own flip and the glass's
    entering-or-leaving test both ask `dot > 0` of exactly this 0."""
    e1 = 2.1e-8
    ray = ((-2.0, -8.0, -8.0), (1.0, 2.0, 2.0))
    cases = []
    # (glass: with a cosine of 0 both branches of the test reflect with probability 1, so they part only where the uniform is
    # exactly 1 -- frame seed 32086816, pixel 0, as in _seeded: entering, the ray refracts; leaving, it reflects totally and goes
    # on along the unset direction)
    for tag, kw, rule, seed in (("", {}, "roty_flip_lax", 1984), ("/glass", dict(mat="glass", ior=1.5), "dielectric_grazing_lax", 32086816)):
        part = moved(quad((-4 - e1, 4 - e1, 1), (8, -8, 0), (2 * e1, 2 * e1, -2), **kw), sg.ROTATE_Y, 90.0)
        cases.append(edge("grazing/normal-perpendicular-to-a-hit" + tag, [(0, part), (1, sphere((30, 40, 40), 9.0))], 0, t=3.0, rules=[rule], ray=ray, tied=[0],
                          seed_base=seed))
    return cases


def _tangent():
    """disc == 0 exactly.  d = (2, 3, -6), a = 49; the sphere of radius 7 around the origin; oc = o - c = (-1, -12, 10) is
    (3, -6, -2) - 2 d, where (3, -6, -2) is perpendicular to d and of length 7: the ray touches the sphere at t = 2.
    b = -2 - 36 - 60 = -98, oc.oc = 245, c = 245 - 49 = 196, disc = 98 * 98 - 49 * 196 = 0: a miss (disc <= 0)."""
    ray = ((-1.0, -12.0, 10.0), (2.0, 3.0, -6.0))
    behind = sphere((9, 3, -20), 6.0)     # the ray's point at t = 5 is its centre: hit squarely, at t = 5 - 6 / 7
    return edge("grazing/tangent-sphere", [(0, sphere((0, 0, 0), 7.0)), (1, behind)], 1, t=None, rules=["sphere_disc_lax"], ray=ray, tied=[], ground=False)


def _media():
    Q = Z0
    wide = box((-40, -40, -3), (40, 40, 0))               # entry in z = 0 at t = 2, exit in z = -3 at t = 2.75, for any o.x
    inside = quad((-40, -40, -1), (80, 0, 0), (0, 80, 0))   # a solid inside the boundary: t = 2.25
    dense = 64.0
    out = [
        # a solid of smaller ordinal exactly on the boundary: the medium's interval [2, 2] is empty; behind it the medium is never seen
        # (an empty interval let through still never scatters unless the scatter distance is 0 too: see the seeded rays below)
        edge("medium/solid-on-entry/before", [(0, Q), (1, fog(wide, dense))], 0, rules=[], tied=[0]),
        edge("medium/solid-on-entry/after", [(0, fog(wide, dense)), (1, Q)], None, t=None, rules=[], tied=[]),
        # a solid inside a dense medium, before and after it in leaf order: clipped to the solid the medium still scatters in front
        edge("medium/solid-inside/before", [(0, inside), (1, fog(wide, dense))], None, t=None, rules=[], tied=[]),
        edge("medium/solid-inside/after", [(0, fog(wide, dense)), (1, inside)], None, t=None, rules=[], tied=[]),
        # two media, each with a tied solid between their ordinals
        edge("medium/two-with-solids", [(0, Q), (1, fog(wide, dense)), (2, Q), (3, fog(SLAB, 0.5)), (4, BALL)], 2, rules=["quad_tmax_strict", "medium_no_tmax_clip"],
             tied=[0, 2, 4]),
        edge("medium/two-with-solids/63-64", [(62, BALL), (63, fog(wide, dense)), (64, Q), (65, fog(SLAB, 0.5))], 64,
             rules=["quad_tmax_strict"], tied=[62, 64], pad=PAD),
    ]
    # The medium's own generator is seeded from the ray: 1337 ^ bits(o.x) ^ bits(o.y * 3.1f) ^ bits(d.z * 5.7f).  With o.y = -4 and
    # d.z = -4 a search of all 2^32 seeds gives these o.x (the plane z = 0 is met at t = 2 whatever
    # o.x is; d.x is then (o.x + 1) - o.x, not 1, which the seed does not read):
    wide_q = quad((-40, -40, 0), (80, 0, 0), (0, 80, 0))
    back = quad((-40, -40, -3), (80, 0, 0), (0, 80, 0))
    u_is_1 = ((5.189828395843506, -4.0, 8.0), D)           # seed 1079383594: the first draw is 0xFFFFFFFF, the uniform exactly 1, log 0
    u_is_small = ((1.5963243246078491, -4.0, 8.0), D)      # seed 1060917602: the first draw is 129, the uniform 3e-8 < 1e-6
    out += [
        # an empty interval and a scatter distance of 0: `rec1.t > rec2.t` would let the medium scatter at t = 2 and, as the later
        # leaf at an equal t, take the pixel from the quad
        edge("medium/empty-interval-distance-0", [(0, wide_q), (1, fog(wide, dense))], 0, rules=["medium_empty_strict"], ray=u_is_1, tied=[0], exact=False),
        edge("medium/uniform-below-floor", [(0, fog(wide, 8.0))], None, t=None, rules=["medium_no_floor"], ray=u_is_small, tied=[], exact=False),
        # hit_distance == distance_inside: along the usual ray the uniform is 0.15301044, log -1.8772491, the interval 0.75 * |d| =
        # 3.4369318, and -1 / density = -1.830834150314331 is the float whose product with the log is that: a scatter, at the exit
        edge("medium/scatter-at-exit", [(0, fog(wide, 0.5461991190345191))], None, t=None, rules=["medium_exit_lax"], tied=[]),
        # ... where a quad lies (z = -3, t = 2.75): a medium's hit at an equal t replaces an earlier record and yields to a later quad
        edge("medium/scatter-on-a-solid/before", [(0, back), (1, fog(wide, 0.5461991190345191))], 1, t=2.75, rules=["medium_exit_lax"]),
        edge("medium/scatter-on-a-solid/after", [(0, fog(wide, 0.5461991190345191)), (1, back)], 1, t=2.75, rules=["quad_tmax_strict"]),
        edge("medium/scatter-on-a-solid/63-64", [(63, back), (64, fog(wide, 0.5461991190345191))], 64, t=2.75, rules=["medium_exit_lax"], pad=PAD),
    ]
    for e in out:
        if e.winner_mat == -1:
            e.winner_mat = None                            # a medium's scatter point is the seed's business, not the design's
    return out


def _textures():
    """A 4 x 2 image of eight distinct texels on spheres hit where u == 1 (atan2 gives pi) and at the poles, under a uv_offset
    that lands on 1, and on emitters; a checker emitter."""
    texels = np.array([[250, 10, 10], [10, 250, 10], [10, 10, 250], [250, 250, 10], [250, 10, 250], [10, 250, 250], [250, 130, 10], [130, 10, 250]], np.uint8)

    def image(b):
        off = len(b.images)
        b.images = np.concatenate([b.images, texels.reshape(-1)])
        return b._tex(sg.T_IMAGE, a=off, b=4, c=2)

    def textured(c, r, how, light=False):
        def make(b, k):
            t = how(b)
            m = b._mat(sg.LIGHT, t, albedo=(9, 9, 9)) if light else b._mat(sg.LAMBERTIAN, t)
            return b.sphere(c, r, m), m
        return make

    # n = (P - c) / r and u = (atan2(-n.z, n.x) + pi) / 2 pi.  Where P.z - c.z = +0 a positive radius gives -n.z = -0, atan2 = -pi
    # and u = 0; a negative radius (a shell, legal in a description) gives n.z = -0, atan2(+0, n.x < 0) = +pi and u == 1 exactly.
    seam = ((-9.0, 0.0, 0.0), (3.0, 0.0, 0.0))             # along x: two zero components (the main kernels and kernel 0; the tier falls back)
    pole_down = ((0.0, 9.0, 0.0), (0.0, -3.0, 0.0))        # meets the north pole of a sphere at the origin: n = (0, 1, 0), v = acos(-1) / pi = 1, row 0
    pole_up = ((0.0, -9.0, 0.0), (0.0, 3.0, 0.0))          # the south pole: v = 0, (1 - v) * h = h: the row clamp
    out = [
        edge("texture/seam", [(0, textured((3, 0, 0), 3.0, image))], 0, t=3.0, rules=[], ray=seam, ground=False, tied=[0]),
        edge("texture/seam-u-1", [(0, textured((3, 0, 0), -3.0, image, light=True))], 0, t=3.0, rules=["image_column_clamp"], ray=((15.0, 0.0, 0.0), (-3.0, 0.0, 0.0)),
             ground=False, tied=[0]),
        edge("texture/north-pole", [(0, textured((0, 0, 0), 3.0, image))], 0, rules=[], ray=pole_down, ground=False, tied=[0]),
        edge("texture/south-pole", [(0, textured((0, 0, 0), 3.0, image))], 0, rules=["image_row_clamp"], ray=pole_up, ground=False, tied=[0]),
        edge("texture/uv-offset-lands-on-1", [(0, textured((0, 0, 0), 3.0, lambda b: b.t_uvoff(image(b), 1.0, 0.5)))], 0, rules=["uvoff_no_wrap"],
             ray=pole_down, ground=False, tied=[0]),
        edge("texture/uv-offset-past-1", [(0, textured((3, 0, 0), 3.0, lambda b: b.t_uvoff(image(b), 1.0, 0.75)))], 0, t=3.0, rules=["uvoff_no_wrap"], ray=seam,
             ground=False, tied=[0]),
        edge("texture/image-light", [(0, textured((0, 0, -3), 3.0, image, light=True))], 0, rules=["light_ignores_texture"], tied=[0]),
        edge("texture/checker-light", [(0, textured((0, 0, -3), 3.0, lambda b: b.t_checker(b.t_solid((4, 1, 1)), b.t_solid((1, 1, 4)), 1.0), light=True))], 0,
             rules=["light_ignores_texture", "checker_parity"], tied=[0]),
        edge("texture/checker", [(0, textured((0, 0, -3), 3.0, lambda b: b.t_checker(b.t_solid((0.9, 0.2, 0.2)), b.t_solid((0.2, 0.2, 0.9)), 1.0)))], 0,
             rules=["checker_parity"], tied=[0]),
    ]
    return out


def _seeded():
    """Rules a random draw decides.  Pixel 0's first sample draws two jitter uniforms, two for the lens disk (accepted at once
    for these seeds) and one for the shutter; the sixth draw on is the material's.  A search of the 2^32 frame seeds gives:
      * 32086816: the sixth draw is 0xFFFFFFFF-ish, a uniform of exactly 1.  A glass quad of ior 0.4 met by the usual ray reflects
        totally (reflect_prob = 1), and `uniform < reflect_prob` is false: the path goes on along the unset refracted
        direction (0, 0, 0), as the reference's does;
      * 1079497666: draws six to eight give a point of the unit sphere whose z is -4 / sqrt(21) = -0.872871518 to the bit, the
        z of the usual ray's unit direction.  On a metal quad in z = 0 with fuzz 1 the scattered direction's z is
        rs.z - u.z = 0: dot(scattered, n) == 0, absorbed."""
    return [edge("seeded/glass-uniform-1", [(0, quad((-2, -2, 0), (4, 0, 0), (0, 4, 0), mat="glass", ior=0.4))], 0, rules=["dielectric_prob_lax"],
                 tied=[0], seed_base=32086816),
            edge("seeded/metal-along-the-surface", [(0, quad((-2, -2, 0), (4, 0, 0), (0, 4, 0), mat="mirror", fuzz=1.0))], 0, rules=["metal_grazing_lax"],
                 tied=[0], seed_base=1079497666)]


def _padded():
    """One tie scene among enough far spheres that the tier kernel reads the scene records from global memory."""
    return [edge("padded/sphere-quad-sphere", [(3, BALL2), (63, Z0), (64, BALL2)], 63, rules=["quad_tmax_strict"], pad=BIG_LEAVES),
            edge("padded/spheres-triple", [(3, BALL), (63, BALL), (64, BALL)], 3, rules=["sphere_tmax_lax"], pad=BIG_LEAVES_LEAN)]


def all_edges():
    return _ties() + _boxes() + _quad_edges() + _grazing() + _media() + _textures() + _seeded()


EDGES = all_edges()
PADDED = _padded()
BY_NAME = {e.name: e for e in EDGES + PADDED}
assert len(BY_NAME) == len(EDGES) + len(PADDED)
