"""Sessions on one resident scene: seeded, replayable sequences of calls, a small model of the description D' the scene should
equal after each of them, and a runner that compares, bit for bit, everything every call writes ("What a scene
carries between calls").

Expected values come from two places.  rt_render frames (their ray counts too), progressive windows, the frame of a variance
call and rt_trace_rays' t, point, normal, uv and material come from the CPU oracle of D' (OracleScene.from_host).  Everything
else -- adaptive frames and their spp maps, variance maps, feature buffers, radiance queries, a trace's prim and inst -- comes
from the same call on a twin: a scene freshly created from D' under the shipped options, made when first needed after a
mutator, anchored by one oracle frame before it is used, closed at the next mutator.

D' is composed with the helpers the update tests use: refit_expect.moved_scene, refit_instances_expect.refit / Moved and
reproject_expect.WithCamera; nothing is computed here.  An op is a plain dict (strings, ints, bools), so that a failing prefix
can be printed, cut down by hand and given to replay().

The runner takes a backend -- the scene factory, the oracle factory, the option calls, device buffers and streams -- so that
tests/test_scene_sessions_host.py can run it on a stub without a device.  Nothing here imports GPU code at module level.
"""
import hashlib

import numpy as np

import accelerated_ray_tracer_amd as art
import refit_expect as rf
import refit_instances_expect as ri
import reproject_expect as rx
import scene_gen as sg

MUTATORS = ("camera", "spheres", "instances", "option")
FRAMES = ("render_plain", "render_ranked", "window", "adaptive", "variance", "aov", "trace", "radiance")
KINDS = MUTATORS + FRAMES
# what may be issued while a non-blocking rt_render is pending (include/rt_abi.h): the scene mutators, rt_render,
# rt_render_adaptive and rt_render_variance finish it first; rt_trace_rays, rt_radiance_rays and the feature-buffer entries
# may run beside it on another stream.  rt_render_window's contract does not say, and rt_set_option is no call on the scene.
MAY_FOLLOW_PENDING = ("camera", "spheres", "instances", "render_plain", "render_ranked", "adaptive", "variance", "aov", "trace", "radiance")
BESIDE_PENDING = ("aov", "trace", "radiance")
KEEPS_PENDING_STATS = ("camera", "spheres", "instances") + BESIDE_PENDING      # the others write statistics of their own
# what an interleaved op between two windows of a progressive frame is drawn from (no mutator, no other progressive frame)
INTERLEAVED = ("render_plain", "render_ranked", "adaptive", "variance", "aov", "trace", "radiance")
# knobs read per frame that schedule and never change a pixel (kernel, bvh_collapse and trace_tree are read at scene creation or
# choose another tree and have tests of their own; lds_mode only with values every scene takes)
OPTIONS = [("split_samples", 2), ("split_samples", 4), ("split_samples", 16), ("handoff", 0), ("handoff", 1), ("cost_map", 0), ("cost_map", 1),
           ("lpt", 0), ("lpt", 1), ("prior", 0), ("prior", 1), ("tier_kernel", 0), ("tier_kernel", 1), ("lds_mode", 0), ("lds_mode", -1),
           ("handoff_pixels", 1 << 24), ("handoff_pixels", -1), ("handoff_poll_us", 1), ("adaptive_tier", 0), ("adaptive_tier", 1)]
RANKED_NS, RANKED_TILES = 32, 64          # the smallest ranked frame (tests/test_cost_map.py): 2 x split_samples, 64 tiles
WINDOW_NS = 8
SEEDS = (1984, 77)
N_RAYS, N_RADIANCE = 2048, 512
FLT_MAX = np.finfo(np.float32).max

# name -> scene, base frame, seed of the walk and number of sequences the walk is cut into (each a GPU test case)
SCENES = {"bouncing": dict(key="bouncing", nx=256, ny=160, seed=11, sequences=5),
          "general": dict(key="general_plain/0", nx=64, ny=64, seed=12, sequences=6),
          "cornell_smoke": dict(key="cornell_smoke", nx=64, ny=64, seed=13, sequences=5),
          "final": dict(key="final", nx=64, ny=64, seed=14, sequences=5)}

_scenes, _generated = {}, {}


def load_scene(name):
    """The base scene of SCENES[name] (host only), made once."""
    if name not in _scenes:
        cfg = SCENES[name]
        if "/" in cfg["key"]:
            recipe, seed = cfg["key"].split("/")
            _scenes[name] = sg.generate(recipe, int(seed), cfg["nx"], cfg["ny"])
        else:
            img, iw, ih = art.default_texture(cfg["key"])
            _scenes[name] = art.HostScene(cfg["key"], cfg["nx"], cfg["ny"], img, iw, ih)
    return _scenes[name]


def movable_spheres(scene):
    return rf.direct_spheres(scene) if scene.desc.n_spheres else np.zeros(0, np.int64)


def followed_instances(scene):
    return ri.followed(scene) if scene.desc.n_instances else np.zeros(0, np.int64)


def supported_kinds(scene):
    """The kinds pair coverage is counted on for this scene: every kind it can take."""
    out = [k for k in KINDS if not (k == "spheres" and len(movable_spheres(scene)) == 0)
           and not (k == "instances" and len(followed_instances(scene)) == 0)]
    return tuple(out)


def geometries(name):
    """name -> (nx, ny, tile_rows, tile_first, tile_stride): the base size, one larger in both dimensions, one much smaller, a
    ragged one (neither dimension a multiple of 8) and a row share of the base size."""
    nx, ny = SCENES[name]["nx"], SCENES[name]["ny"]
    return {"base": (nx, ny, ny, 0, 1), "large": (nx + 32, ny + 24, ny + 24, 0, 1), "small": (24, 16, 16, 0, 1),
            "ragged": (nx - 13, ny - 9, ny - 9, 0, 1), "share": (nx, ny, 8, 1, 2)}


def local_rows(geom):
    """Global rows of the frame a geometry assigns to the call, in local order (rt_frame_local_rows' rule)."""
    nx, ny, tile_rows, first, stride = geom
    return np.array([r for r in range(ny) if (r // tile_rows) % stride == first], np.int64)


def tiles(geom):
    """8 x 8 tiles of the local frame, rounded down: no ranked frame is asked for where rounding could decide."""
    return (geom[0] // 8) * (len(local_rows(geom)) // 8)


def cameras(scene):
    """Four cameras: the scene's own, the eye and the frame shifted together, the shifted one zoomed in, and a shift the other
    way.  Fields are moved as float32 vectors; any finite camera is one the ABI and the oracle take."""
    base = scene.desc.camera
    h, v = np.array(base.horizontal, np.float32), np.array(base.vertical, np.float32)

    def made(shift, zoom):
        c = art.RtCamera.from_buffer_copy(base)
        d = (np.float32(shift[0]) * h + np.float32(shift[1]) * v).astype(np.float32)
        inset = np.float32(0.5 * (1 - zoom))
        c.origin[:] = np.array(base.origin, np.float32) + d
        c.lower_left_corner[:] = np.array(base.lower_left_corner, np.float32) + d + inset * h + inset * v
        c.horizontal[:] = np.float32(zoom) * h
        c.vertical[:] = np.float32(zoom) * v
        return c
    return [art.RtCamera.from_buffer_copy(base), made((0.15, 0.1), 1.0), made((0.15, 0.1), 0.8), made((-0.2, 0.05), 1.0)]


def query_rays(scene):
    """N_RAYS rays from around the base camera's eye, half through its frame and half towards points of the scene's root box,
    with times in the shutter."""
    cam = scene.desc.camera
    rng = np.random.default_rng(5)
    n = N_RAYS
    eye, h, v = np.array(cam.origin, np.float64), np.array(cam.horizontal, np.float64), np.array(cam.vertical, np.float64)
    o = eye + rng.uniform(-0.05, 0.05, (n, 3)) * np.linalg.norm(v)
    s, t = rng.uniform(0, 1, (2, n, 1))
    through = np.array(cam.lower_left_corner, np.float64) + s * h + t * v
    root = scene.nodes()[0]
    lo, hi = np.maximum(root["bmin"].astype(np.float64), eye - 50), np.minimum(root["bmax"].astype(np.float64), eye + 50)
    inside = lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)
    target = np.where((np.arange(n) % 2 == 0)[:, None], through, inside)
    d = (target - o).astype(np.float32)
    d[(d == 0).all(1)] = 1.0
    tm = (cam.time0 + rng.uniform(0, 1, n) * (cam.time1 - cam.time0)).astype(np.float32)
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d), tm


def _camera_bytes(c):
    b = bytearray(bytes(c))
    off = type(c).pad.offset
    b[off:off + 4] = b"\0" * 4
    return bytes(b)


def records_key(camera, spheres, instances):
    """What tells two descriptions over one base scene apart: the camera and the sphere and instance records."""
    h = hashlib.sha1()
    for part in (_camera_bytes(camera), np.ascontiguousarray(spheres).tobytes(), np.ascontiguousarray(instances).tobytes()):
        h.update(part)
        h.update(b"|")
    return h.hexdigest()[:16]


def desc_records(desc):
    """(sphere records, instance records) a description points to, copied."""
    import ctypes as C
    out = []
    for ptr, n, dtype in ((desc.spheres, desc.n_spheres, art.SPHERE_DTYPE), (desc.instances, desc.n_instances, art.INSTANCE_DTYPE)):
        out.append(np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(ptr), dtype, n).copy() if n else np.zeros(0, dtype))
    return out


def desc_key(scene):
    return records_key(scene.desc.camera, *desc_records(scene.desc))


# ----------------------------------------------------------------------------- the model
class Model:
    """D' = (camera, sphere records, instance records) over a fixed base scene, and the options in force."""

    def __init__(self, base):
        self.base = base
        self.records = base          # the base scene with every sphere and instance update applied, under its own camera
        self.cams = cameras(base)
        self.cam = 0
        self.options = []            # (key, value) in the order set since the last reset
        self.version = 0
        self._scene = None

    def scene(self):
        """D' as a scene description (anything with HostScene's surface)."""
        if self._scene is None:
            self._scene = rx.WithCamera(art, self.records, self.cams[self.cam])
        return self._scene

    def key(self):
        return desc_key(self.scene())

    def legal_updates(self, kind):
        """The update kinds of the helpers' UPDATES that D' can take now."""
        if kind == "spheres":
            return list(rf.UPDATES)
        inst = self.records.instances()
        ids = followed_instances(self.records)
        flags = inst["flags"][ids]
        has_flags = bool(((flags == ri.TRANSLATE) | (flags == (ri.ROTATE_Y | ri.TRANSLATE))).any())
        return [u for u in ri.UPDATES if u != "flags" or has_flags]

    def update_of(self, op):
        """(indices or None, first, records) of a `spheres` / `instances` op on D' as it stands.  With op["first"] the update
        is cut down to its longest run of consecutive indices, sorted, and given as a range."""
        mod = rf if op["kind"] == "spheres" else ri
        idx, rec = mod.make_update(self.records, op["update"])
        idx = np.asarray(idx, np.int64)
        if not op["first"]:
            return idx, 0, rec
        order = np.argsort(idx, kind="stable")
        idx, rec = idx[order], rec[order]
        best, start = (0, 1), 0
        for k in range(1, len(idx) + 1):
            if k == len(idx) or idx[k] != idx[k - 1] + 1:
                if k - start > best[1] - best[0]:
                    best = (start, k)
                start = k
        return None, int(idx[best[0]]), rec[best[0]:best[1]]

    def apply(self, op, update=None):
        """A mutator: D' after it.  `update`: what update_of(op) gave (it is taken on D' before the op)."""
        kind = op["kind"]
        if kind == "option":
            if op.get("reset"):
                self.options = []
            else:
                self.options = [kv for kv in self.options if kv[0] != op["key"]] + [(op["key"], op["value"])]
            return
        if kind == "camera":
            self.cam = op["cam"]
        else:
            idx, first, rec = update if update is not None else self.update_of(op)
            idx = np.arange(first, first + len(rec)) if idx is None else idx
            if kind == "spheres":
                self.records = rf.moved_scene(self.records, idx, rec)
            else:
                nodes, inst, _, _ = ri.refit(self.records, idx, rec)
                self.records = ri.Moved(self.records, nodes, inst)
        self.version += 1
        self._scene = None


# ----------------------------------------------------------------------------- the generator
def _circuit(kinds, rng):
    """A closed walk over `kinds` that takes every ordered pair, self-pairs included, exactly once (Hierholzer on the complete
    digraph with loops): len(kinds)^2 + 1 kinds."""
    out = {k: [kinds[j] for j in rng.permutation(len(kinds))] for k in kinds}
    stack, walk = ["render_plain"], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def _pick(rng, items):
    return items[int(rng.integers(len(items)))]


def _frame_op(kind, name, rng, nxt=None, turn=None):
    """One non-mutating op of `kind` (not `window`) with its parameters drawn.  nxt: the kind that follows, if known: a ranked
    frame in front of a scene mutator is always left pending, in front of another op that may follow one mostly.  turn: the
    sequence's count of `aov` ops so far, in a list: rt_render_aov and rt_render_aov_through alternate."""
    geoms = geometries(name)
    op = {"kind": kind}
    if kind in ("trace", "radiance"):
        return op
    if kind == "render_ranked":
        op["geom"] = _pick(rng, [g for g in geoms if tiles(geoms[g]) >= RANKED_TILES])
        pending = nxt in MAY_FOLLOW_PENDING and (nxt in MUTATORS or rng.random() < 0.6)
        op["mode"] = "pending" if pending else _pick(rng, ["blocking", "finish"])
    else:
        op["geom"] = _pick(rng, list(geoms))
    op["seed"] = _pick(rng, SEEDS)
    if kind == "render_plain":
        op["ns"] = _pick(rng, [1, 6])
        op["device"] = bool(rng.integers(2))
    elif kind == "adaptive":
        op["threshold"] = _pick(rng, [0.05, 0.2])
    elif kind == "aov":
        op["through"] = bool(turn[0] % 2)
        turn[0] += 1
    return op


def _mutator_op(kind, model, rng):
    if kind == "camera":
        return {"kind": kind, "cam": int((model.cam + rng.integers(1, 4)) % 4), "recalibrate": int(rng.integers(2))}      # another one
    if kind == "option":
        if rng.random() < 0.15:
            return {"kind": kind, "reset": True}
        key, value = _pick(rng, OPTIONS)
        return {"kind": kind, "key": key, "value": value}
    device = bool(rng.integers(2))
    return {"kind": kind, "update": _pick(rng, model.legal_updates(kind)), "first": bool(rng.integers(2)), "device": device,
            "side": bool(device and rng.integers(2)), "recalibrate": int(rng.integers(2))}


def _emit(name, kind, nxt, model, rng, turn):
    """The ops of one kind of the walk: one op, or for `window` 2-4 window ops with other non-mutating ops between them."""
    if kind in MUTATORS:
        op = _mutator_op(kind, model, rng)
        model.apply(op)
        return [op]
    if kind != "window":
        return [_frame_op(kind, name, rng, nxt, turn)]
    ops = []
    geom, seed = _pick(rng, list(geometries(name))), _pick(rng, SEEDS)
    ends = sorted(int(e) for e in rng.choice(np.arange(1, WINDOW_NS), int(rng.integers(1, 4)), replace=False)) + [WINDOW_NS]
    begin = 0
    for w, end in enumerate(ends):
        ops.append({"kind": "window", "geom": geom, "seed": seed, "begin": begin, "end": end, "last": end == WINDOW_NS})
        begin = end
        if end != WINDOW_NS:
            for _ in range(int(rng.integers(1, 3)) if w == 0 else int(rng.integers(0, 2))):
                ops.append(_frame_op(_pick(rng, INTERLEAVED), name, rng, None, turn))
    return ops


def _cut(name, walk, target):
    """The walk as sequences of `target` ops or a few more: a sequence ends with the kind the next one starts with, so no pair
    of the walk falls into a cut.  Each sequence starts from the base scene.  The walk is closed; a last sequence that would
    be short goes round again until it has SEQUENCE_OPS[0] ops."""
    cfg, base = SCENES[name], load_scene(name)
    rng = np.random.default_rng([cfg["seed"], 2])
    sequences, model, ops, turn = [], Model(base), [], [0]
    for p, kind in enumerate(walk):
        nxt = walk[p + 1] if p + 1 < len(walk) else None
        if nxt is not None and ops and len(ops) + 1 >= target:
            ops += _emit(name, kind, None, model, rng, turn)
            sequences.append(ops)
            model, ops, turn = Model(base), [], [0]
        ops += _emit(name, kind, nxt if nxt is not None else walk[1], model, rng, turn)
    p = 1
    while len(ops) < SEQUENCE_OPS[0]:
        ops += _emit(name, walk[p], walk[p + 1] if len(ops) + 1 < SEQUENCE_OPS[0] else None, model, rng, turn)
        p += 1
    sequences.append(ops)
    return sequences


SEQUENCE_OPS = (30, 45)
TARGET_OPS = 36          # a progressive frame adds at most 8 ops to a sequence that has reached it


def generate(name):
    """The sequences of SCENES[name]: a walk that takes every ordered pair of the scene's kinds once, cut into sequences of
    30-45 ops, each kind turned into ops with parameters drawn from the scene's seed.  Deterministic; made once."""
    if name not in _generated:
        walk = _circuit(supported_kinds(load_scene(name)), np.random.default_rng([SCENES[name]["seed"], 1]))
        _generated[name] = _cut(name, walk, TARGET_OPS)
    return _generated[name]


def pairs(ops):
    """The ordered pairs of kinds adjacent in `ops`.  Two windows of one progressive frame with nothing between them are one
    `window`, not a self-pair; an op drawn between two windows follows `window`, and the next window follows it."""
    out = set()
    for a, b in zip(ops, ops[1:]):
        if a["kind"] == "window" and b["kind"] == "window" and b["begin"] != 0:
            continue
        out.add((a["kind"], b["kind"]))
    return out


def check_legal(name, ops):
    """Every op of a sequence is one its scene takes, in a place where the contracts cover it; AssertionError otherwise."""
    base = load_scene(name)
    kinds, geoms = supported_kinds(base), geometries(name)
    model, open_window, pending = Model(base), None, False
    for i, op in enumerate(ops):
        kind = op["kind"]
        assert kind in kinds, (i, op)
        assert not pending or kind in MAY_FOLLOW_PENDING, (i, op, "follows a pending frame")
        pending = False
        if kind in MUTATORS:
            assert open_window is None, (i, op, "a mutator inside a progressive frame")
            if kind in ("spheres", "instances"):
                assert op["update"] in model.legal_updates(kind), (i, op)
                idx, first, rec = model.update_of(op)
                idx = np.arange(first, first + len(rec)) if idx is None else idx
                assert len(rec) > 0 and len(np.unique(idx)) == len(idx)
                if kind == "spheres":
                    assert np.isin(idx, movable_spheres(model.records)).all(), (i, op, "a sphere under an instance")
                else:
                    assert idx.min() >= 0 and idx.max() < model.records.desc.n_instances
                    assert np.array_equal(rec["child"], model.records.instances()["child"][idx])
                model.apply(op, (idx, 0, rec))
            else:
                if kind == "camera":
                    assert 0 <= op["cam"] < 4
                elif not op.get("reset"):
                    assert (op["key"], op["value"]) in OPTIONS
                model.apply(op)
            continue
        if "geom" in op:
            assert op["geom"] in geoms, (i, op)
        if kind == "render_ranked":
            assert tiles(geoms[op["geom"]]) >= RANKED_TILES, (i, op, "a ranked frame under 64 tiles")
            assert op["mode"] in ("blocking", "finish", "pending")
            pending = op["mode"] == "pending"
        if kind == "window":
            if op["begin"] == 0:
                assert open_window is None, (i, op)
            else:
                assert open_window == (op["geom"], op["seed"], op["begin"]), (i, op, "windows must follow each other")
            assert op["begin"] < op["end"] <= WINDOW_NS and op["last"] == (op["end"] == WINDOW_NS)
            open_window = None if op["last"] else (op["geom"], op["seed"], op["end"])
        elif open_window is not None:
            assert kind in INTERLEAVED, (i, op)


# ----------------------------------------------------------------------------- the runner
class Mismatch(AssertionError):
    def __init__(self, text, step=None):
        super().__init__(text)
        self.step = step


class SessionFailure(AssertionError):
    """A session that did not give what the model expects; .step is the op's index, .prefix the ops up to and including it."""

    def __init__(self, text, step, prefix):
        super().__init__(text)
        self.step, self.prefix = step, prefix


def _digest(x):
    if isinstance(x, np.ndarray):
        return hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]
    return repr(x)


class GpuBackend:
    """The backend of the real thing: DeviceScene, the oracle, torch for device buffers and streams."""

    def __init__(self, gpu, orc):
        self.art, self.orc = gpu, orc

    def create(self, host):
        return self.art.DeviceScene(host)

    def oracle(self, host):
        return self.orc.OracleScene.from_host(host)

    def set_option(self, key, value):
        self.art.set_option(key, value)

    def reset_options(self):
        self.art.reset_options()

    def node_boxes(self, ds):
        """rt_debug_scene_boxes, array 0: (bmin, bmax) of the reference tree as it stands on the device."""
        import ctypes as C
        L, n = self.art.rt_lib(), C.c_size_t(0)
        assert L.rt_debug_scene_boxes(ds._p, 0, None, 0, C.byref(n)) == 0
        out = np.zeros(n.value // self.art.NODE_DTYPE.itemsize, self.art.NODE_DTYPE)
        assert L.rt_debug_scene_boxes(ds._p, 0, out.ctypes.data, out.nbytes, C.byref(n)) == 0
        return out["bmin"], out["bmax"]

    def ranked(self, ds):
        state, _, parts = ds.cost_map()
        return state == "exact" and parts in (1, 2)

    def buffer(self, shape):
        import torch
        t = torch.zeros(shape, dtype=torch.float32, device=torch.device("cuda", self.art._initialised_device or 0))
        torch.cuda.synchronize()
        return _TorchBuffer(t)

    def records(self, rec):
        import torch
        return torch.from_numpy(np.ascontiguousarray(rec).view(np.float32).reshape(-1, 8).copy()).to(torch.device("cuda", self.art._initialised_device or 0))

    def stream(self):
        import torch
        return torch.cuda.Stream()


class _TorchBuffer:
    def __init__(self, t):
        self.t, self.ptr = t, t.data_ptr()

    def numpy(self):
        return self.t.cpu().numpy()


class Session:
    """One resident scene, its model, its twin and what was compared so far.  run() drives it."""

    def __init__(self, name, backend, label=None):
        self.name, self.backend, self.label = name, backend, label or name
        self.base = load_scene(name)
        self.geoms = geometries(name)
        self.model = Model(self.base)
        self.rays = query_rays(self.base)
        self.ds = backend.create(self.base)
        self.twin = None
        self.oracle = None
        self.cache = {}              # expected values of the current D' version
        self.window = None           # [the open progressive frame, its rays so far]
        self.pending = None          # (step, buffer, stream, the oracle's frame, rays, samples) of a frame left pending
        self.mutators = []           # (step, op) of every mutator so far
        self.log = []                # per step: [(what, digest)]
        self.keys = []               # per step: desc_key of D' after it
        self._key = self.model.key()
        self.step = -1
        self.twins_made = 0

    # ---- comparisons
    def same(self, got, want, what, step=None):
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        if got.shape != want.shape or got.dtype != want.dtype:
            raise Mismatch(f"{what}: shape / dtype {got.shape} {got.dtype}, expected {want.shape} {want.dtype}", step)
        a = got.view(np.uint8) if got.dtype.itemsize == 1 else got.view(np.uint32)
        b = want.view(np.uint8) if want.dtype.itemsize == 1 else want.view(np.uint32)
        bad = np.argwhere(a != b)
        if len(bad):
            raise Mismatch(f"{what}: {len(bad)} of {a.size} values differ, first at {bad[:3].tolist()}: "
                           f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}", step)
        self.log[-1 if step is None else step].append((what, _digest(got)))

    def values(self, got, want, what):
        """Equal as floats (so +0 == -0), no NaN on either side."""
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape or np.isnan(got).any() or np.isnan(want).any():
            raise Mismatch(f"{what}: shapes {got.shape} and {want.shape}, or a NaN")
        bad = np.argwhere(got != want)
        if len(bad):
            raise Mismatch(f"{what}: {len(bad)} of {got.size} values differ, first at {bad[:3].tolist()}: "
                           f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")
        self.log[-1].append((what, _digest(got)))

    def equal(self, got, want, what, step=None):
        if got != want:
            raise Mismatch(f"{what}: {got!r} != {want!r}", step)
        self.log[-1 if step is None else step].append((what, repr(got)))

    # ---- expected values
    def frame(self, geom, ns, seed):
        nx, ny, rows, first, stride = self.geoms[geom]
        return self.model.scene().frame(nx=nx, ny=ny, ns=ns, seed_base=seed, tile_rows=rows, tile_first=first, tile_stride=stride)

    def _oracle(self):
        if self.oracle is None:
            self.oracle = self.backend.oracle(self.model.scene())
        return self.oracle

    def oracle_frame(self, geom, ns, seed):
        """(the local rows of the oracle's frame, its rays) for D' as it stands; a row share is rendered band by band."""
        key = ("oracle", geom, ns, seed)
        if key not in self.cache:
            nx, ny, tile_rows, first, stride = self.geoms[geom]
            o = self._oracle()
            o.nx, o.ny = nx, ny
            rows = local_rows(self.geoms[geom])
            if len(rows) == ny:
                fb, cnt = o.render(ns, seed_base=seed)
                self.cache[key] = (fb, cnt["rays"])
            else:
                fb, rays = np.zeros((ny, nx, 3), np.float32), 0
                for r0 in sorted(set(int(r) // tile_rows * tile_rows for r in rows)):
                    band, cnt = o.render(ns, seed_base=seed, row0=r0, row1=min(r0 + tile_rows, ny))
                    fb[r0:r0 + tile_rows] = band[r0:r0 + tile_rows]
                    rays += cnt["rays"]
                self.cache[key] = (np.ascontiguousarray(fb[rows]), rays)
        return self.cache[key]

    def oracle_trace(self):
        if "trace" not in self.cache:
            o, d, tm = self.rays
            t, p, n, uv, mat = self._oracle().trace(o, d, tm)
            hit = t < FLT_MAX
            assert hit.sum() * 4 >= len(o), f"{self.label}: only {int(hit.sum())} of {len(o)} query rays hit the scene"
            self.cache["trace"] = dict(t=t, point=p, normal=n, uv=uv, mat=mat, hit=hit)
        return self.cache["trace"]

    def on_twin(self, key, call):
        """What `call` gives on the twin, under the shipped options; made once per D' version and key."""
        key = ("twin",) + key
        if key not in self.cache:
            if self.model.options:
                self.backend.reset_options()
            try:
                if self.twin is None:
                    self.twin = self.backend.create(self.model.scene())
                    self.twins_made += 1
                    # the twin is anchored by the oracle before it is used
                    fb, st = self.twin.render(self.frame("base", 1, SEEDS[0]))
                    want, rays = self.oracle_frame("base", 1, SEEDS[0])
                    self.same(fb, want, "the twin's anchor frame against the oracle")
                    self.equal(int(st.rays), rays, "the twin's anchor frame: rays")
                self.cache[key] = call(self.twin)
            finally:
                for k, v in self.model.options:
                    self.backend.set_option(k, v)
        return self.cache[key]

    def _new_version(self):
        if self.twin is not None:
            self.twin.close()
            self.twin = None
        self.oracle = None
        self.cache = {}

    # ---- a pending frame
    def settle_pending(self, keeps_stats):
        """The frame left pending by an earlier step: its buffer, and its statistics where the op after it left them alone.
        A mismatch belongs to the step that issued the frame."""
        if self.pending is None:
            return
        step, buf, stream, want, rays, samples = self.pending
        self.pending = None
        if keeps_stats:
            st = self.ds.finish()
            self.equal(int(st.rays), rays, "the pending frame's rays after finish()", step)
            self.equal(int(st.samples), samples, "the pending frame's samples after finish()", step)
        stream.synchronize()
        self.same(buf.numpy(), want, "the pending frame's buffer", step)

    # ---- the ops
    def do(self, i, op):
        kind = op["kind"]
        self.step = i
        self.log.append([])
        if kind in MUTATORS:
            self.mutate(op)
            self.mutators.append((i, op))
            self._key = self.model.key()
        else:
            getattr(self, "op_" + kind)(op)
        self.keys.append(self._key)
        if self.pending is not None and self.pending[0] != i:      # the frame an earlier step left pending
            self.settle_pending(kind in KEEPS_PENDING_STATS)

    def mutate(self, op):
        kind, ds, m = op["kind"], self.ds, self.model
        if kind == "option":
            if op.get("reset"):
                self.backend.reset_options()
            else:
                self.backend.set_option(op["key"], op["value"])
            m.apply(op)
            self.log[-1].append(("options in force", repr(m.options)))
            return
        if kind == "camera":
            ds.set_camera(m.cams[op["cam"]], recalibrate=bool(op["recalibrate"]))
            m.apply(op)
            self.equal(_camera_bytes(ds.camera()) == _camera_bytes(m.cams[op["cam"]]), True, "the scene's camera after set_camera")
        else:
            update = m.update_of(op)
            idx, first, rec = update
            stream = self.backend.stream() if op["side"] else None
            given = self.backend.records(rec) if op["device"] else rec
            call = ds.update_spheres if kind == "spheres" else ds.update_instances
            call(given, idx, first=first, recalibrate=bool(op["recalibrate"]), stream=stream)
            m.apply(op, update)
            got = ds.spheres() if kind == "spheres" else ds.instances()
            want = m.records.spheres() if kind == "spheres" else m.records.instances()
            self.equal(got.tobytes() == want.tobytes(), True, f"the scene's {kind} records after the update")
            boxes = self.backend.node_boxes(ds)      # the reference tree's boxes on the device, where the backend can read them
            if boxes is not None:
                nodes = m.records.nodes()
                for k, have in zip(("bmin", "bmax"), boxes):
                    self.values(have, nodes[k], f"the scene's node boxes ({k}) after the update, by value")
        self._new_version()

    def _rendered(self, fb, st, geom, ns, seed, what):
        want, rays = self.oracle_frame(geom, ns, seed)
        self.same(fb, want, f"{what}: frame against the oracle")
        self.equal(int(st.rays), rays, f"{what}: rays against the oracle")
        self.equal(int(st.samples), want.shape[0] * want.shape[1] * ns, f"{what}: samples")
        self.equal(int(st.local_rows), want.shape[0], f"{what}: local rows")

    def op_render_plain(self, op):
        f = self.frame(op["geom"], op["ns"], op["seed"])
        if op["device"]:
            rows = len(local_rows(self.geoms[op["geom"]]))
            buf = self.backend.buffer((rows, f.nx, 3))
            _, st = self.ds.render(f, out=buf.ptr)
            fb = buf.numpy()
        else:
            fb, st = self.ds.render(f)
        self._rendered(fb, st, op["geom"], op["ns"], op["seed"], "render_plain")

    def op_render_ranked(self, op):
        f = self.frame(op["geom"], RANKED_NS, op["seed"])
        if op["mode"] == "blocking":
            fb, st = self.ds.render(f)
            self._rendered(fb, st, op["geom"], RANKED_NS, op["seed"], "render_ranked")
            opts = dict(self.model.options)
            if opts.get("lpt", 1) and opts.get("cost_map", 1):      # the frame did take the ranked path this op is about
                self.equal(self.backend.ranked(self.ds), True, "render_ranked: the frame ran ranked and left its cost map")
            return
        # what the frame must be is settled now: a mutator may follow before it is looked at
        want, rays = self.oracle_frame(op["geom"], RANKED_NS, op["seed"])
        earlier = self.pending
        buf, stream = self.backend.buffer(want.shape), self.backend.stream()
        self.ds.render(f, out=buf.ptr, stream=stream.cuda_stream, blocking=False)        # (finishes an earlier pending frame first)
        mine = (self.step, buf, stream, want, rays, want.shape[0] * want.shape[1] * RANKED_NS)
        if earlier is not None:
            self.pending = earlier
            self.settle_pending(False)
        self.pending = mine
        if op["mode"] == "finish":
            self.settle_pending(True)

    def op_window(self, op):
        if op["begin"] == 0:
            self.close_window()
            self.window = [self.ds.progressive(self.frame(op["geom"], WINDOW_NS, op["seed"])), 0]
        pf = self.window[0]
        fb, st = pf.render(op["begin"], op["end"])
        want, rays = self.oracle_frame(op["geom"], op["end"], op["seed"])
        self.window[1] += int(st.rays)
        self.same(fb, want, f"window [{op['begin']}, {op['end']}): frame against the oracle's {op['end']}-sample frame")
        self.equal(self.window[1], rays, f"window [{op['begin']}, {op['end']}): rays so far against the oracle")
        if op["last"]:
            self.close_window()

    def close_window(self):
        if self.window is not None:
            self.window[0].close()
            self.window = None

    def op_adaptive(self, op):
        f = self.frame(op["geom"], WINDOW_NS, op["seed"])
        call = lambda s: s.render_adaptive(f, 2, 8, op["threshold"])   # noqa: E731
        got = call(self.ds)
        want = self.on_twin(("adaptive", op["geom"], op["seed"], op["threshold"]), call)
        self.same(got[0], want[0], "adaptive: frame against the twin")
        self.same(got[1], want[1], "adaptive: spp map against the twin")
        self.equal((int(got[2].rays), int(got[2].samples)), (int(want[2].rays), int(want[2].samples)), "adaptive: rays and samples")
        self.equal(int(got[2].samples), int(got[1].astype(np.int64).sum()), "adaptive: samples against the spp map")

    def op_variance(self, op):
        f = self.frame(op["geom"], 4, op["seed"])
        call = lambda s: s.render_variance(f, 2)   # noqa: E731
        got = call(self.ds)
        want = self.on_twin(("variance", op["geom"], op["seed"]), call)
        self._rendered(got[0], got[2], op["geom"], 4, op["seed"], "variance")
        self.same(got[0], want[0], "variance: frame against the twin")
        self.same(got[1], want[1], "variance: variance map against the twin")
        self.equal((int(got[2].rays), int(got[2].samples)), (int(want[2].rays), int(want[2].samples)), "variance: rays and samples")

    def op_aov(self, op):
        f = self.frame(op["geom"], 4, op["seed"])
        if op["through"]:
            call = lambda s: s.render_aov_through(f, ids=True, through=True, bounces=True)   # noqa: E731
        else:
            call = lambda s: s.render_aov(f, ids=True)   # noqa: E731
        got = call(self.ds)
        want = self.on_twin(("aov", op["geom"], op["seed"], op["through"]), call)
        self.equal(sorted(got), sorted(want), "aov: outputs")
        for k in sorted(want):
            self.same(got[k], want[k], f"aov{'_through' if op['through'] else ''}: {k} against the twin")

    def op_trace(self, op):
        o, d, tm = self.rays
        want = self.oracle_trace()
        got = self.ds.trace(o, d, tm, record=True)
        for k in ("t", "point", "normal", "uv", "mat"):
            self.same(getattr(got, k), want[k], f"trace: {k} against the oracle")
        self.same(got.prim >= 0, want["hit"], "trace: hits against the oracle")
        twin = self.on_twin(("trace",), lambda s: s.trace(o, d, tm, record=True))
        for k in ("prim", "inst"):
            self.same(getattr(got, k), getattr(twin, k), f"trace: {k} against the twin")
        self.same(np.asarray(self.ds.trace(o, d, tm, any_hit=True)), want["hit"], "trace: any-hit against the oracle")

    def op_radiance(self, op):
        o, d, tm = (x[:N_RADIANCE] for x in self.rays)
        call = lambda s: s.radiance(o, d, tm, ns=2, count_rays=True)   # noqa: E731
        got, want = call(self.ds), self.on_twin(("radiance",), call)
        self.same(got.rgb, want.rgb, "radiance: rgb against the twin")
        self.same(got.rays, want.rays, "radiance: rays against the twin")

    def close(self):
        try:
            self.close_window()
            if self.pending is not None:
                self.ds.finish()
                self.pending[2].synchronize()
                self.pending = None
        finally:
            if self.twin is not None:
                self.twin.close()
                self.twin = None
            self.ds.close()


def run(session, ops):
    """Executes `ops` on the session, updating the model as it goes and comparing after every op.  Returns the session's log:
    per step the list of (what was compared, a digest of it).  A mismatch raises SessionFailure."""
    try:
        i = -1
        try:
            for i, op in enumerate(ops):
                session.do(i, op)
            i = len(ops) - 1
            session.settle_pending(True)
        except Mismatch as m:
            step = i if m.step is None else m.step
            prefix = [dict(o) for o in ops[:max(step, i) + 1]]
            last = [x for x in session.mutators if x[0] < step]
            seen = "" if step == i else f"\n  (a frame left pending: seen while step {i}, op {ops[i]!r}, was checked)"
            text = (f"session {session.label} (scene {session.name}, seed {SCENES[session.name]['seed']}): step {step}, op {ops[step]!r}\n"
                    f"  {m}{seen}\n"
                    f"  the last mutator before it: {'none' if not last else f'step {last[-1][0]}, {last[-1][1]!r}'}\n"
                    f"  D' version {session.model.version}, options in force {session.model.options!r}\n"
                    f"  to see it again: session_expect.replay({session.name!r}, {prefix!r}, backend)")
            raise SessionFailure(text, step, prefix) from None
    finally:
        try:
            session.close()
        finally:
            session.backend.reset_options()
    return session.log


def replay(name, prefix, backend):
    """Runs `prefix` -- a list of ops as a failure report prints it, or any cut of it that check_legal takes -- on a new scene."""
    check_legal(name, prefix)
    return run(Session(name, backend, f"{name}/replay"), prefix)
