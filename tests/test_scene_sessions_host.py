"""The session test's own parts, without a device (tests/session_expect.py): the generator is deterministic, covers every
ordered pair of kinds on every scene and emits only ops the contracts cover; the model's D' equals, version by version, what
the host-only rt_refit_nodes / rt_refit_instances give when each is applied to the description the previous one produced; and
the runner, on a stub scene whose outputs are a cheap function of (D', op, parameters), passes every sequence and catches each
of four planted history bugs at the first step where it is visible, naming that step."""
import hashlib
import types

import numpy as np
import pytest

import refit_expect as rf
import refit_instances_expect as ri
import session_expect as se

SCENE_NAMES = list(se.SCENES)
N_KINDS = {"bouncing": 11, "general": 12, "cornell_smoke": 11, "final": 11}      # bouncing holds no instance, cornell_smoke no sphere, final no instance a leaf follows


# ----------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_generator_is_deterministic_covers_every_pair_and_is_legal(art, name):
    first = se.generate(name)
    se._generated.pop(name)
    again = se.generate(name)
    assert first == again and first is not again
    kinds = se.supported_kinds(se.load_scene(name))
    assert len(kinds) == N_KINDS[name], kinds
    assert len(first) == se.SCENES[name]["sequences"]
    covered = set()
    for ops in first:
        assert 30 <= len(ops) <= 45, len(ops)
        se.check_legal(name, ops)
        covered |= se.pairs(ops)
        # every cached frame buffer is both grown and under-filled within the sequence
        sizes = [np.prod(_shape(name, op)) for op in ops if "geom" in op]
        steps = np.sign(np.diff(sizes))
        assert (steps > 0).any() and (steps < 0).any()
        through = [op["through"] for op in ops if op["kind"] == "aov"]
        assert through == [bool(k % 2) for k in range(len(through))]          # rt_render_aov and rt_render_aov_through alternate
    missing = {(a, b) for a in kinds for b in kinds} - covered
    assert not missing, sorted(missing)
    assert len({(a, b) for a in kinds for b in kinds}) == N_KINDS[name] ** 2
    everything = [op for ops in first for op in ops]
    assert {op["mode"] for op in everything if op["kind"] == "render_ranked"} == {"blocking", "finish", "pending"}
    assert any(a["kind"] == "render_ranked" and a["mode"] == "pending" and b["kind"] in se.MUTATORS for ops in first for a, b in zip(ops, ops[1:]))
    assert any(a["kind"] == "render_ranked" and a["mode"] == "pending" and b["kind"] in se.BESIDE_PENDING for ops in first for a, b in zip(ops, ops[1:]))
    assert {op["geom"] for op in everything if "geom" in op} == set(se.geometries(name))


def test_the_alphabet_is_what_the_issue_asks_for(art):
    assert len(se.KINDS) == 12 and len({k for k, _ in se.OPTIONS}) >= 6
    assert not {"kernel", "bvh_collapse", "trace_tree"} & {k for k, _ in se.OPTIONS}
    for name in SCENE_NAMES:
        g = se.geometries(name)
        nx, ny = se.SCENES[name]["nx"], se.SCENES[name]["ny"]
        assert g["base"][:2] == (nx, ny) and g["large"][0] > nx and g["large"][1] > ny and g["small"][0] * g["small"][1] * 8 <= nx * ny
        assert g["ragged"][0] % 8 and g["ragged"][1] % 8 and g["share"][2:] == (8, 1, 2)
        assert any(se.tiles(x) >= se.RANKED_TILES for x in g.values())
    # the local rows of a geometry are the library's
    lib = se.art.rt_lib()
    for geom in se.geometries("bouncing").values():
        f = se.load_scene("bouncing").frame(nx=geom[0], ny=geom[1], ns=1, tile_rows=geom[2], tile_first=geom[3], tile_stride=geom[4])
        assert np.array_equal(se.local_rows(geom), se.art.local_rows_to_global(f)), geom
    assert lib is not None


def test_an_illegal_sequence_is_refused(art):
    ops = [{"kind": "render_ranked", "geom": "small", "seed": 1984, "mode": "blocking"}]
    with pytest.raises(AssertionError, match="64 tiles"):
        se.check_legal("general", ops)
    ops = [{"kind": "render_ranked", "geom": "base", "seed": 1984, "mode": "pending"},
           {"kind": "window", "geom": "base", "seed": 1984, "begin": 0, "end": 8, "last": True}]
    with pytest.raises(AssertionError, match="pending"):
        se.check_legal("general", ops)
    with pytest.raises(AssertionError):
        se.check_legal("bouncing", [{"kind": "instances", "update": "one", "first": False, "device": False, "side": False, "recalibrate": 0}])


def _shape(name, op):
    geom = se.geometries(name)[op["geom"]]
    return (len(se.local_rows(geom)), geom[0])


# ----------------------------------------------------------------------------- the model against the library's host statements
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_model_composes_as_the_host_refits_do(art, name):
    """Every mutator of every sequence, one after the other: rt_refit_nodes / rt_refit_instances on the description the
    previous step produced give the model's nodes, spheres and instances by value, at every version."""
    base = se.load_scene(name)
    versions = 0
    for ops in se.generate(name):
        model, cur = se.Model(base), base
        for op in ops:
            if op["kind"] not in se.MUTATORS:
                continue
            if op["kind"] in ("spheres", "instances"):
                idx, first, rec = update = model.update_of(op)
                if op["kind"] == "spheres":
                    nodes, records = art.refit_nodes(cur.desc, rec, idx, first)
                    cur = rf.Moved(cur, nodes, records)
                else:
                    nodes, records = art.refit_instances(cur.desc, rec, idx, first)
                    cur = ri.Moved(cur, nodes, records)
                model.apply(op, update)
                versions += 1
            else:
                model.apply(op)
            got, want = model.records.nodes(), cur.nodes()
            assert np.array_equal(got["skip"], want["skip"]) and np.array_equal(got["prim"], want["prim"])
            rf.same_values(got["bmin"], want["bmin"], f"{name} bmin after {op}")
            rf.same_values(got["bmax"], want["bmax"], f"{name} bmax after {op}")
            assert ri.scene_spheres(model.records).tobytes() == ri.scene_spheres(cur).tobytes()
            assert model.records.instances().tobytes() == cur.instances().tobytes()
            d = model.scene().desc
            assert se._camera_bytes(d.camera) == se._camera_bytes(model.cams[model.cam])
            sph, inst = se.desc_records(d)
            assert sph.tobytes() == ri.scene_spheres(cur).tobytes() and inst.tobytes() == cur.instances().tobytes()
    assert versions >= 8


# ----------------------------------------------------------------------------- the runner on a stub
def _rng(*parts):
    return np.random.default_rng(int.from_bytes(hashlib.sha1(repr(parts).encode()).digest()[:8], "little"))


def _frame_values(key, nx, ny, ns, seed):
    return _rng(key, "frame", nx, ny, ns, seed).random((ny, nx, 3), dtype=np.float32)


def _row_rays(key, nx, ny, seed):
    return _rng(key, "rays", nx, ny, seed).integers(1, 50, ny)


def _trace_values(key, n):
    r = _rng(key, "trace", n)
    hit = r.random(n) < 0.6
    t = np.where(hit, r.random(n, dtype=np.float32) + np.float32(0.5), se.FLT_MAX).astype(np.float32)
    vec = lambda c: (r.random((n, c), dtype=np.float32) * hit[:, None]).astype(np.float32)   # noqa: E731
    return dict(t=t, point=vec(3), normal=vec(3), uv=vec(2), mat=np.where(hit, r.integers(0, 5, n), -1).astype(np.int32),
                prim=np.where(hit, r.integers(0, 99, n), -1).astype(np.int32), inst=np.where(hit, r.integers(-1, 3, n), -1).astype(np.int32))


class StubOracle:
    def __init__(self, key):
        self.key, self.nx, self.ny = key, 0, 0

    def render(self, ns, seed_base=1984, row0=0, row1=None):
        row1 = self.ny if row1 is None else row1
        fb = np.zeros((self.ny, self.nx, 3), np.float32)
        fb[row0:row1] = _frame_values(self.key, self.nx, self.ny, ns, seed_base)[row0:row1]
        return fb, {"rays": int(_row_rays(self.key, self.nx, self.ny, seed_base)[row0:row1].sum()) * ns}

    def trace(self, o, d, tm):
        v = _trace_values(self.key, len(o))
        return v["t"], v["point"], v["normal"], v["uv"], v["mat"]


class StubStream:
    cuda_stream = 7

    def synchronize(self):
        pass


class StubBuffer:
    def __init__(self, shape, ptr):
        self.a, self.ptr = np.zeros(shape, np.float32), ptr

    def numpy(self):
        return self.a.copy()


class StubRecords:
    """Device-resident records: anything but a numpy array."""

    def __init__(self, rec):
        self.rec = rec.copy()


class StubBackend:
    """Scenes whose outputs are a function of (D', op, parameters).  `defect`: the history bug planted in the first scene
    made -- the resident one; the twins, which have no history, are sound."""

    def __init__(self, defect=None):
        self.defect, self.buffers, self.scenes, self.option_calls = defect, {}, 0, []

    def create(self, host):
        self.scenes += 1
        return StubScene(self, host, self.defect if self.scenes == 1 else None)

    def oracle(self, host):
        return StubOracle(se.desc_key(host))

    def set_option(self, key, value):
        self.option_calls.append((key, value))

    def reset_options(self):
        self.option_calls.append("reset")

    def buffer(self, shape):
        b = StubBuffer(shape, 4096 + 16 * len(self.buffers))
        self.buffers[b.ptr] = b
        return b

    def records(self, rec):
        return StubRecords(rec)

    def ranked(self, ds):
        return True

    def node_boxes(self, ds):
        return None      # (the stub keeps no tree)

    def stream(self):
        return StubStream()


class StubScene:
    def __init__(self, backend, host, defect):
        self.backend, self.defect = backend, defect
        self.cam = se.art.RtCamera.from_buffer_copy(host.desc.camera)
        self.sph, self.inst = se.desc_records(host.desc)
        self.pending, self.stale_key, self.last_stats = False, None, None
        self.cache, self.prev_floats = np.zeros(0, np.float32), 0        # the cached frame buffer of host frames
        self.spp_cache = None
        self.calls = 0

    # ---- state
    def key(self):
        self.calls += 1
        if self.stale_key is not None:          # (planted) one output of the description before the update
            k, self.stale_key = self.stale_key, None
            return k
        return se.records_key(self.cam, self.sph, self.inst)

    def _mutating(self):
        if self.pending and self.defect == "stale" and self.stale_key is None:
            self.stale_key = se.records_key(self.cam, self.sph, self.inst)
        self.pending = False

    def set_camera(self, camera, recalibrate=False):
        self._mutating()
        self.cam = se.art.RtCamera.from_buffer_copy(camera)

    def _update(self, mine, records, indices, first):
        self._mutating()
        rec = records.rec if isinstance(records, StubRecords) else records
        idx = np.arange(first, first + len(rec)) if indices is None else np.asarray(indices)
        mine[idx] = rec

    def update_spheres(self, records, indices=None, first=0, recalibrate=False, stream=None):
        assert (stream is None) or isinstance(records, StubRecords)
        self._update(self.sph, records, indices, first)

    def update_instances(self, records, indices=None, first=0, recalibrate=False, stream=None):
        assert (stream is None) or isinstance(records, StubRecords)
        self._update(self.inst, records, indices, first)

    def camera(self):
        return self.cam

    def spheres(self):
        return self.sph.copy()

    def instances(self):
        return self.inst.copy()

    # ---- frames
    @staticmethod
    def _geom(f):
        return (f.nx, f.ny, f.tile_rows, f.tile_first, f.tile_stride)

    def _frame(self, f, ns, key=None):
        rows = se.local_rows(self._geom(f))
        key = self.key() if key is None else key
        fb = np.ascontiguousarray(_frame_values(key, f.nx, f.ny, ns, f.seed_base)[rows])
        rays = int(_row_rays(key, f.nx, f.ny, f.seed_base)[rows].sum())
        return fb, rays, rows

    def _through_host_cache(self, fb):
        """A host frame passes through the cached device frame buffer, which is grown and never shrunk."""
        n = fb.size
        out = fb.copy()
        if self.defect == "rows" and self.prev_floats > n:      # (planted) the last row keeps what the larger frame left there
            out[-1] = self.cache[n - out[-1].size:n].reshape(out[-1].shape)
        if len(self.cache) < n:
            self.cache = np.zeros(n, np.float32)
        self.cache[:n] = fb.ravel()
        self.prev_floats = n
        return out

    def _stats(self, rays, samples, rows):
        self.last_stats = types.SimpleNamespace(rays=rays, samples=samples, local_rows=rows)
        return self.last_stats

    def render(self, f, out=None, stream=0, blocking=True):
        self.pending = False
        fb, rays, rows = self._frame(f, f.ns)
        st = self._stats(rays * f.ns, len(rows) * f.nx * f.ns, len(rows))
        if out is None:
            return self._through_host_cache(fb), st
        self.backend.buffers[out].a[...] = fb
        self.pending = not blocking
        return None, st

    def finish(self):
        self.pending = False
        return self.last_stats

    def progressive(self, f):
        return StubProgressive(self, f)

    def render_adaptive(self, f, min_spp, max_spp, threshold):
        self.pending = False
        key = self.key()
        fb, _, rows = self._frame(f, max_spp, key)
        spp = _rng(key, "spp", self._geom(f), f.seed_base, threshold).choice(np.array([2, 4, 8], np.int32), (len(rows), f.nx))
        self.spp_cache = spp.ravel().copy()
        return self._through_host_cache(fb), spp, self._stats(int(spp.sum()) * 3, int(spp.sum()), len(rows))

    def render_variance(self, f, batches):
        self.pending = False
        key = self.key()
        fb, rays, rows = self._frame(f, f.ns, key)
        var = _rng(key, "variance", self._geom(f), f.seed_base).random((len(rows), f.nx), dtype=np.float32)
        if self.defect == "spp" and self.spp_cache is not None and self.spp_cache.size >= var.size:      # (planted) the borrowed buffer
            var = self.spp_cache[:var.size].view(np.float32).reshape(var.shape).copy()
        return self._through_host_cache(fb), var, self._stats(rays * f.ns, len(rows) * f.nx * f.ns, len(rows))

    def _aov(self, f, names, what):
        key = self.key()
        rows = len(se.local_rows(self._geom(f)))
        r = _rng(key, what, self._geom(f), f.ns, f.seed_base)
        return {k: (r.random((rows, f.nx, 3), dtype=np.float32) if k in ("albedo", "normal") else
                    r.integers(-1, 9, (rows, f.nx)).astype(np.int32) if k in ("prim", "inst", "mat", "bounces") else
                    r.random((rows, f.nx), dtype=np.float32)) for k in names}

    def render_aov(self, f, ids=False):
        return self._aov(f, ["albedo", "normal", "depth", "alpha", "prim", "inst", "mat"], "aov")

    def render_aov_through(self, f, ids=False, through=False, bounces=False):
        return self._aov(f, ["albedo", "normal", "depth", "alpha", "prim", "inst", "mat", "through", "bounces"], "aov_through")

    def trace(self, o, d, tm, record=False, any_hit=False):
        v = _trace_values(self.key(), len(o))
        return v["t"] < se.FLT_MAX if any_hit else types.SimpleNamespace(**v)

    def radiance(self, o, d, tm, ns=1, count_rays=False):
        r = _rng(self.key(), "radiance", len(o), ns)
        return types.SimpleNamespace(rgb=r.random((len(o), 3), dtype=np.float32), rays=r.integers(1, 99, len(o)).astype(np.int32))

    def close(self):
        pass


class StubProgressive:
    def __init__(self, scene, f):
        self.scene, self.f, self.first_end, self.calls_then, self.forgot = scene, f, None, None, False

    def render(self, begin, end):
        s = self.scene
        if s.defect == "window" and begin > 0 and s.calls != self.calls_then:      # (planted) another call came between two windows
            self.forgot = True
        fb, rays, rows = s._frame(self.f, end - self.first_end if self.forgot else end)
        if begin == 0:
            self.first_end = end
        self.calls_then = s.calls
        return s._through_host_cache(fb), s._stats(rays * (end - begin), len(rows) * self.f.nx * (end - begin), len(rows))

    def close(self):
        pass


def _host_frame(op):
    return (op["kind"] in ("window", "adaptive", "variance") or (op["kind"] == "render_plain" and not op["device"])
            or (op["kind"] == "render_ranked" and op["mode"] == "blocking"))


def _first_visible(name, ops, keys, defect):
    """The first step at which the planted defect changes something the runner looks at, or None."""
    floats = lambda op: int(np.prod(_shape(name, op))) * 3   # noqa: E731
    if defect == "stale":
        for i in range(1, len(ops)):
            if ops[i]["kind"] in ("camera", "spheres", "instances") and ops[i - 1]["kind"] == "render_ranked" and ops[i - 1]["mode"] == "pending":
                j = next((j for j in range(i + 1, len(ops)) if ops[j]["kind"] not in se.MUTATORS), None)
                if j is not None and keys[j] != keys[i - 1]:
                    return j
                if j is not None:
                    continue
        return None
    if defect == "rows":
        prev = 0
        for i, op in enumerate(ops):
            if _host_frame(op):
                if prev > floats(op):
                    return i
                prev = floats(op)
        return None
    if defect == "spp":
        pixels = None
        for i, op in enumerate(ops):
            if op["kind"] == "adaptive":
                pixels = floats(op) // 3
            if op["kind"] == "variance" and pixels is not None and pixels >= floats(op) // 3:
                return i
        return None
    assert defect == "window"
    for i, op in enumerate(ops):
        if op["kind"] == "window" and op["begin"] > 0 and ops[i - 1]["kind"] != "window":
            return i
    return None


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_sound_stub_passes_every_sequence(art, name):
    for k, ops in enumerate(se.generate(name)):
        backend = StubBackend()
        s = se.Session(name, backend, f"{name}-{k}")
        log = se.run(s, ops)
        assert len(log) == len(ops) == len(s.keys) and all(len(entry) > 0 for entry in log)
        assert backend.option_calls[-1] == "reset"
        mutators = sum(op["kind"] in ("camera", "spheres", "instances") for op in ops)
        assert 1 <= s.twins_made <= mutators + 1                       # made lazily, closed at the next mutator
        # ... and a replay of the first half gives the same log
        half = ops[:len(ops) // 2]
        while half and half[-1]["kind"] == "render_ranked" and half[-1]["mode"] == "pending":
            half = half[:-1]
        again = se.replay(name, half, StubBackend())
        assert again == log[:len(half)]


@pytest.mark.parametrize("defect", ["stale", "rows", "spp", "window"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_planted_history_bug_is_caught_at_its_first_step(art, name, defect):
    caught = 0
    for k, ops in enumerate(se.generate(name)):
        sound = se.Session(name, StubBackend(), f"{name}-{k}")
        se.run(sound, ops)
        want = _first_visible(name, ops, sound.keys, defect)
        s = se.Session(name, StubBackend(defect), f"{name}-{k}")
        if want is None:
            se.run(s, ops)
            continue
        with pytest.raises(se.SessionFailure) as e:
            se.run(s, ops)
        assert e.value.step == want, (k, defect, e.value.step, want, str(e.value))
        text = str(e.value)
        assert f"step {want}, op {ops[want]!r}" in text and f"scene {name}, seed {se.SCENES[name]['seed']}" in text
        assert "values differ, first at" in text and "the last mutator before it" in text
        assert e.value.prefix[:want + 1] == ops[:want + 1] and repr(e.value.prefix) in text
        # the printed prefix is one replay() takes, and it fails at the same step
        prefix = eval(text.split("session_expect.replay(")[1].rsplit(", backend)", 1)[0].split(", ", 1)[1])   # noqa: S307 (our own repr)
        assert prefix == e.value.prefix
        with pytest.raises(se.SessionFailure) as e2:
            se.replay(name, prefix, StubBackend(defect))
        assert e2.value.step == want
        caught += 1
    assert caught >= 1, f"no sequence of {name} shows the planted '{defect}' defect"
