"""What rt_render_aov_through must return (include/rt_abi.h, "feature buffers through mirrors and glass"), predicted from the CPU
oracle and a NumPy float32 restatement of the chain's few lines of vector arithmetic.

The primary rays are the oracle's ray sample of the emissive twin, as tests/aov_expect.py takes them.  Then, for k = 0 ..
max_bounces, OracleScene.trace walks the rays that are still live in the ORIGINAL scene; each hit is classified by the
description's material array; a followed hit's next direction is formed below in float32 -- every operation a NumPy float32
ufunc, rounded once, nothing fused, sums left to right as the contract writes them -- and the next ray starts at the oracle's hit
point.  The terminal normal, t and material are the oracle's.

The terminal albedo is independent NumPy wherever it can be: a terminal hit whose material carries an inline colour (tex < 0, or a
metal, or glass) and a terminal miss under a constant background.  For the rest -- a textured terminal material, the gradient
miss term -- this module LEANS ON PRODUCT CODE: DeviceScene.radiance at ns = 1 of the emissive twin along the chain's last ray,
which is the twin's emitted colour at the first hit or the miss term (pinned against the oracle by tests/test_radiance.py), times
the tint.  Without a device (tests/test_aov_through_host.py) those samples' albedo is left NaN and counted in "device_needed".

Also here, shared by the host and the GPU tests: the scenes, frames and parameters of the GPU test.
"""
from __future__ import annotations

import numpy as np

import aov_expect as ax
import scene_gen as sg

F = np.float32
FLT_MAX = ax.FLT_MAX
FUZZ_LIMIT = 0.5                 # the tests' limit: scene_gen's metals have fuzz 0, 1 and one in between
BOUNCES = (1, 2, 8)
SPHERES, GENERAL = ax.PARITY[0], "final"          # spheres_plain: glass (a hollow shell among it), mirrors, fuzzy metals
GENERAL2 = ax.PARITY[3]                           # general_plain: quads, boxes and instances beside glass and a mirror
NO_GLASS, NO_GLASS_FUZZ_LIMIT = "built/no_glass", 0.125   # build_no_glass(): every metal's fuzz is above this limit
FRAMES = [(ax.NX, ax.NY, 1), (ax.NX, ax.NY, 4), (13, 9, 4)]
SHARE = dict(tile_rows=4, tile_first=1, tile_stride=2)


def build_no_glass(nx=ax.NX, ny=ax.NY):
    """A glass-free description: a checkered ground, two fuzzy metal spheres (fuzz 0.25 and 1), a matte one and a metal quad."""
    rng = np.random.default_rng(11)
    b = sg.Builder(rng)
    b.leaf(sg._ground(b, b.t_checker(b.t_solid(), b.t_solid(), 0.5)))
    b.leaf(b.sphere((-1.6, 0.8, 0.0), 0.8, b.metal(0.25)))
    b.leaf(b.sphere((0.2, 0.7, 0.8), 0.7, b.metal(1.0)))
    b.leaf(b.sphere((1.9, 0.6, -0.4), 0.6, b.lambertian()))
    b.leaf(b.quad((-3.0, 0.0, -2.5), (6.0, 0.0, 0.0), (0.0, 2.5, 0.0), b.metal(0.5)))
    return b.finish("no_glass", sg._camera(rng, nx, ny), nx, ny, gradient=1, background=(0.3, 0.35, 0.5))


def pdot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(F)


def unit(d):
    length = np.sqrt(pdot(d, d)).astype(F)
    return (d / length[:, None]).astype(F), length


def mirror(u, n):
    c2 = (F(2) * pdot(u, n)).astype(F)
    return (u - (c2[:, None] * n).astype(F)).astype(F)


def through_glass(d, u, n, ior):
    """-> (d', total internal reflection)"""
    inside = pdot(d, n) > 0
    m = np.where(inside[:, None], -n, n).astype(F)
    with np.errstate(divide="ignore"):
        e = np.where(inside, ior, (F(1) / ior).astype(F)).astype(F)
    dt = pdot(u, m)
    disc = (F(1) - ((e * e).astype(F) * (F(1) - (dt * dt).astype(F)).astype(F)).astype(F)).astype(F)
    with np.errstate(invalid="ignore"):
        s = np.sqrt(np.where(disc > 0, disc, F(0))).astype(F)
    inner = (u - (dt[:, None] * m).astype(F)).astype(F)
    refr = ((e[:, None] * inner).astype(F) - (s[:, None] * m).astype(F)).astype(F)
    tir = ~(disc > 0)
    return np.where(tir[:, None], mirror(u, n), refr).astype(F), tir


def chain(whole, mats, rays, max_bounces, fuzz_limit):
    """The chains of the primary rays `rays` ((n, 8), trace_families.ray_sample) in the oracle scene `whole`, per sample:
    k, tint, hit / t / normal / mat of the terminal event, depth, the last ray (o, d, tm), and what happened on the way -- tir
    (some total internal reflection was followed), cut (ended by max_bounces on a hit that would have been followed),
    metal_followed / metal_unfollowed (some metal hit of the chain was / was not followed because of its fuzz)."""
    n = len(rays)
    o, d, tm = rays[:, 0:3].astype(F).copy(), rays[:, 3:6].astype(F).copy(), rays[:, 6].astype(F).copy()
    _, len0 = unit(d)
    r = {"k": np.zeros(n, np.int32), "tint": np.ones((n, 3), F), "hit": np.zeros(n, bool), "t": np.zeros(n, F), "normal": np.zeros((n, 3), F),
         "mat": np.full(n, -1, np.int32), "depth": np.zeros(n, F)}
    for key in ("tir", "cut", "metal_followed", "metal_unfollowed", "metal_back"):
        r[key] = np.zeros(n, bool)
    t0, tsum = np.zeros(n, F), np.zeros(n, F)
    live = np.arange(n)
    fuzz_limit = F(fuzz_limit)
    for step in range(max_bounces + 1):
        if len(live) == 0:
            break
        t, p, nrm, _, mat = whole.trace(o[live], d[live], tm[live])
        hit = t < FLT_MAX
        kind = np.where(hit, mats["kind"][np.where(hit, mat, 0)], -1)
        fuzz = mats["fuzz"][np.where(hit, mat, 0)].astype(F)
        ior = mats["ior"][np.where(hit, mat, 0)].astype(F)
        metal, glass = kind == sg.METAL, kind == sg.DIELECTRIC
        would = glass | (metal & (fuzz <= fuzz_limit))
        r["metal_unfollowed"][live] |= metal & ~(fuzz <= fuzz_limit)
        u, _ = unit(d[live])
        refl = mirror(u, nrm)
        back = metal & would & ~(pdot(nrm, refl) > 0)
        r["metal_back"][live] |= back & (step < max_bounces)
        with np.errstate(invalid="ignore", divide="ignore"):
            refr, tir = through_glass(d[live], u, nrm, np.where(glass, ior, F(1)).astype(F))
        follow = would & ~back & (step < max_bounces)
        r["cut"][live] |= would & ~back & (step == max_bounces)
        r["tir"][live] |= follow & glass & tir
        r["metal_followed"][live] |= follow & metal
        # terminal events
        end = live[~follow]
        e = ~follow
        r["hit"][end], r["t"][end], r["mat"][end] = hit[e], np.where(hit[e], t[e], F(0)), np.where(hit[e], mat[e], -1)
        r["normal"][end] = np.where(hit[e][:, None], nrm[e], F(0))
        if step == 0:
            r["depth"][end] = np.where(hit[e], t[e], F(0))
        else:
            far = (t0[end] + ((tsum[end] + t[e]).astype(F) / len0[end]).astype(F)).astype(F)
            r["depth"][end] = np.where(hit[e], far, F(0))
        # followed hits: ray k + 1
        go = live[follow]
        if step == 0:
            t0[go] = t[follow]
        else:
            tsum[go] = (tsum[go] + t[follow]).astype(F)
        m_go = metal[follow]
        r["tint"][go[m_go]] = (r["tint"][go[m_go]] * mats["albedo"][mat[follow][m_go]].astype(F)).astype(F)
        r["k"][go] += 1
        o[go] = p[follow]
        d[go] = np.where(m_go[:, None], refl[follow], refr[follow])
        assert np.isfinite(d[go]).all() and np.isfinite(o[go]).all()
        live = go
    assert len(live) == 0 or step == max_bounces
    r["last_o"], r["last_d"], r["last_tm"] = o, d, tm
    return r


def expected(case, nx, ny, ns, max_bounces, fuzz_limit=FUZZ_LIMIT, twin_ds=None):
    """Every output of the whole nx x ny frame of `case` (an aov_expect.Case) at ns samples and seed_base ax.SEED, and the
    per-sample chain records (shape (ny, nx, ns, ...)) under "chain".  twin_ds: a DeviceScene of case.twin, for the albedo of
    textured terminals and of the gradient miss term; None leaves those samples' albedo NaN."""
    base = case.expect(ns, nx, ny)
    scene = case.scene
    mats = scene.materials()
    media = scene.media() if scene.desc.n_media else np.zeros(0, sg.art.MEDIUM_DTYPE)
    # the pass never follows a medium hit; the classification below goes by the material alone, so no medium may carry a specular one
    assert not np.isin(mats["kind"][media["mat"]], [sg.METAL, sg.DIELECTRIC]).any()
    whole = case._orc.OracleScene.from_host(scene, nx, ny)
    c = chain(whole, mats, base["rays"], max_bounces, fuzz_limit)
    n = len(base["rays"])
    # the terminal albedo before the tint
    hit, mat = c["hit"], np.where(c["hit"], c["mat"], 0)
    kind, tex = mats["kind"][mat], mats["tex"][mat]
    inline = hit & ((tex < 0) | (kind == sg.METAL) | (kind == sg.DIELECTRIC))
    alb = np.full((n, 3), np.nan, F)
    alb[inline] = np.where((kind[inline] == sg.DIELECTRIC)[:, None], F(1), mats["albedo"][mat[inline]]).astype(F)
    flat_miss = ~hit & (not scene.use_gradient_bg)
    alb[flat_miss] = np.asarray(scene.background, F)
    need = ~(inline | flat_miss)
    if twin_ds is not None and need.any():
        rgb = twin_ds.radiance(np.ascontiguousarray(c["last_o"][need]), np.ascontiguousarray(c["last_d"][need]),
                               np.ascontiguousarray(c["last_tm"][need]), ns=1, background=scene.background, gradient=scene.use_gradient_bg).rgb
        alb[need] = rgb
    alb = (c["tint"] * alb).astype(F)
    shape = (ny, nx, ns)
    per = {k: v.reshape(shape + v.shape[1:]) for k, v in c.items()}
    return {"albedo": ax._sum_samples(alb.reshape(shape + (3,)), ns), "normal": ax._sum_samples(per["normal"], ns),
            "depth": ax._sum_samples(per["depth"], ns), "alpha": ax._sum_samples(per["hit"].astype(F), ns),
            "through": ax._sum_samples((per["k"] >= 1).astype(F), ns), "mat": per["mat"][:, :, 0].copy(), "bounces": per["k"][:, :, 0].copy(),
            "chain": per, "device_needed": need.reshape(shape), "first": base}


class Cases:
    """aov_expect.Case by scene and the expectations of this module by (scene, frame, max_bounces, fuzz_limit): computed once,
    left unchanged.  twin_scene(key): the DeviceScene of the twin, made by the GPU test; None on the host."""

    def __init__(self, art, orc, twin_scene=None):
        self._art, self._orc, self._twin_scene = art, orc, twin_scene
        self._cases, self._cache = {}, {}

    def case(self, key):
        if key not in self._cases:
            if key == NO_GLASS:
                c = ax.Case.__new__(ax.Case)
                c.key, c.scene = key, build_no_glass()
                c.twin, c._art, c._orc, c._cache = ax.Twin(self._art, c.scene), self._art, self._orc, {}
                self._cases[key] = c
            else:
                self._cases[key] = ax.Case(self._art, self._orc, key)
        return self._cases[key]

    def expect(self, key, nx, ny, ns, max_bounces, fuzz_limit=FUZZ_LIMIT):
        k = (key, nx, ny, ns, max_bounces, float(fuzz_limit))
        if k not in self._cache:
            twin = self._twin_scene(key) if self._twin_scene else None
            self._cache[k] = expected(self.case(key), nx, ny, ns, max_bounces, fuzz_limit, twin)
        return self._cache[k]
