"""rt_reproject_quads / reproject(quads=...) / TemporalAccumulator(follow_quads=True) on the GPU.  Every comparison is bit for bit
against the NumPy restatement of the extended contract (tests/reproject_quads_expect.py), NaNs compared as equal: out, out_len and
motion, on seeded synthetic buffers whose ids, inst planes and tables reach every branch of the three follow steps, at a size that
is no multiple of the tile, on small frames, on the identities with rt_reproject_instances and rt_reproject, on real pairs of
frames between which quads and boxes moved, from host arrays and device tensors, on a side stream, and through the accumulator."""
import ctypes as C

import numpy as np
import pytest

import reproject_expect as rx
import reproject_instances_expect as ix
import reproject_quads_expect as qx

pytestmark = pytest.mark.gpu

NX, NY = 37, 29            # three tiles by two, neither a multiple of 16
TIGHT = dict(alpha_min=0.75, depth_tol=0.0, normal_min=0.9, max_history=4.0)
_cache = {}


def _synthetic():
    if "synthetic" not in _cache:
        _cache["synthetic"] = qx.synthetic_quads(NX, NY, 7)
    return _cache["synthetic"]


def _assert_same(got, want, what):
    got = np.ascontiguousarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs in other places"
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def _check(result, want, what, motion=True):
    _assert_same(result.out, want[0], what + " out")
    _assert_same(result.length, want[1], what + " out_len")
    if motion:
        _assert_same(result.motion, want[2], what + " motion")
    else:
        assert result.motion is None


@pytest.mark.parametrize("motion", [False, True])
@pytest.mark.parametrize("normals", [False, True])
def test_synthetic_buffers_every_branch_of_the_three_follow_steps(gpu, normals, motion):
    """The inputs tests/test_reproject_quads_host.py counts the branches of, under a previous camera a few degrees away, the same
    camera, and one the points are behind (a <= 0); then the tight thresholds, the ranges' ends among them."""
    s = _synthetic()
    kw, t = qx.select(s["buffers"], normals), s["tables"]
    for name, prev in s["cams"].items():
        want = qx.reproject(cur=s["cur"], prev=prev, **kw, **t)
        got = gpu.reproject(cur=s["cur"], prev=prev, motion=motion, **kw, **t)
        _check(got, want, f"{name} normals={normals}", motion)
        want = qx.reproject(cur=s["cur"], prev=prev, **kw, **t, **TIGHT)
        _check(gpu.reproject(cur=s["cur"], prev=prev, motion=motion, **kw, **t, **TIGHT), want, f"{name} tight thresholds", motion)


@pytest.mark.parametrize("nx,ny", [(1, 1), (16, 16), (17, 1), (1, 33)])
def test_small_and_tile_sized_frames(gpu, nx, ny):
    s = qx.synthetic_quads(nx, ny, 100 * nx + ny)
    for prev in s["cams"].values():
        _check(gpu.reproject(cur=s["cur"], prev=prev, motion=True, **s["buffers"], **s["tables"]),
               qx.reproject(cur=s["cur"], prev=prev, **s["buffers"], **s["tables"]), f"{nx}x{ny}")


def test_identities_with_the_other_entries(gpu):
    """Unmoved quad tables (record 5 still differing in n, w, D, mat and the pads) and empty ones against rt_reproject_instances on
    the painted planes with the moving sphere and instance tables; with nothing moved and inst = -1 everywhere against rt_reproject
    -- the device's own bits of the same buffers for every camera --, through the binding and through the C entry with
    descriptions of nothing but zeros, the planes and the quad tables.  A null history: out == color and out_len == 1, with the
    followed motion still written."""
    s = _synthetic()
    t, b = s["tables"], s["buffers"]
    rest = qx.without_quads(t)
    cur, same = qx.unmoved_quad_tables()
    empty = np.zeros(0, gpu.QUAD_DTYPE)
    none = np.full((NY, NX), -1, np.int32)
    bn = dict(b, inst=none, prev_inst=none)
    plain = ix.without_inst(bn)
    L = gpu.rt_lib()
    for name, prev in s["cams"].items():
        instances = tuple(np.ascontiguousarray(x) for x in gpu.reproject(cur=s["cur"], prev=prev, motion=True, **b, **rest))
        _check(gpu.reproject(cur=s["cur"], prev=prev, motion=True, quads=cur, prev_quads=same, **b, **rest), instances, f"{name} unmoved quad tables")
        _check(gpu.reproject(cur=s["cur"], prev=prev, motion=True, quads=empty, prev_quads=empty, **b, **rest), instances, f"{name} empty quad tables")
        static = tuple(np.ascontiguousarray(x) for x in gpu.reproject(cur=s["cur"], prev=prev, motion=True, **plain))
        _check(gpu.reproject(cur=s["cur"], prev=prev, motion=True, quads=cur, prev_quads=same, **bn), static, f"{name} nothing moved, no instance")
        d, m, im, qm = gpu.RtReprojectDesc(), gpu.RtReprojectMotionDesc(), gpu.RtReprojectInstanceDesc(), gpu.RtReprojectQuadDesc()
        d.nx, d.ny, d.cur, d.prev = NX, NY, s["cur"], prev
        out, out_len, mot = np.full((NY, NX, 3), -7, np.float32), np.full((NY, NX), -7, np.float32), np.full((NY, NX, 2), -7, np.float32)
        for k, v in dict(plain, out=out, out_len=out_len, motion=mot).items():
            setattr(d, k, v.ctypes.data)
        d.alpha_min, d.depth_tol, d.normal_min, d.max_history = (rx.DEFAULTS[k] for k in ("alpha_min", "depth_tol", "normal_min", "max_history"))
        im.inst, im.prev_inst = none.ctypes.data, none.ctypes.data
        qm.n_quads, qm.quads, qm.prev_quads = len(cur), cur.ctypes.data, same.ctypes.data
        assert L.rt_reproject_quads(C.byref(d), C.byref(m), C.byref(im), C.byref(qm), 0, None, 1) == 0, L.rt_last_error_detail().decode()
        _check(gpu.ReprojectResult(out, out_len, mot), static, f"{name} the C entry, unmoved quads, n_instances = 0, n_spheres = 0")
    first = gpu.reproject(b["color"], b["depth"], b["alpha"], s["cur"], s["cams"]["near"], normal=b["normal"], prim=b["prim"],
                          prev_normal=b["prev_normal"], prev_prim=b["prev_prim"], inst=b["inst"], motion=True, **t)
    assert np.array_equal(first.out.view(np.uint32), b["color"].view(np.uint32))
    assert np.array_equal(first.length, np.ones((NY, NX), np.float32))
    _assert_same(first.motion, qx.reproject(cur=s["cur"], prev=s["cams"]["near"], **b, **t)[2], "first frame motion")
    unfollowed = gpu.reproject(b["color"], b["depth"], b["alpha"], s["cur"], s["cams"]["near"], prim=b["prim"], prev_prim=b["prev_prim"],
                               inst=b["inst"], motion=True, **rest)
    assert not np.array_equal(first.motion, unfollowed.motion, equal_nan=True)


# --------------------------------------------------------------------------------------------------------- real pairs
def _resized(gpu, quads, first, scale, mat=None):
    """The six records of the box at quads[first : first + 6] with its extent scaled per axis about its low corner."""
    a, b = qx.box_extent(quads[first:first + 6])
    b2 = (a + (b - a) * np.asarray(scale, np.float32)).astype(np.float32)
    return gpu.box_records(a, b2, int(quads["mat"][first]) if mat is None else mat)


def _moved_cornell(gpu, quads, instances):
    """The short block (quads 3..8, under instance 0) made a third taller while its instance turns by 6 degrees, and the light
    (quad 17) slid by a sixth of its length along its u."""
    light = quads[17:18].copy()
    light["Q"] = (light["Q"] + light["u"] / np.float32(6)).astype(np.float32)
    light = gpu.quad_record(light["Q"][0], light["u"][0], light["v"][0], int(light["mat"][0]))
    idx = np.array(list(range(3, 9)) + [17], np.int32)
    return idx, np.concatenate([_resized(gpu, quads, 3, (1.0, 4.0 / 3.0, 1.0)), light]), np.array([0], np.int32), ix.turned(instances, [0], 6.0)


def _moved_quads(gpu, quads, instances):
    """Quad 1 (the back wall) translated by (0.3, 0.2, 0) and quad 2 (the floor) sheared: its u gains 0.15 of its v."""
    back = gpu.quad_record(quads["Q"][1] + np.array([0.3, 0.2, 0.0], np.float32), quads["u"][1], quads["v"][1], int(quads["mat"][1]))
    floor = gpu.quad_record(quads["Q"][2], quads["u"][2] + np.float32(0.15) * quads["v"][2], quads["v"][2], int(quads["mat"][2]))
    return np.array([1, 2], np.int32), np.concatenate([back, floor]), None, None


def _moved_instanced(gpu, quads, instances):
    """Every box that sits under an instance made a quarter wider, a fifth lower and a tenth deeper, and every quad that sits
    directly under an instance slid by a tenth of its u -- the instances stand still, so each carry happens in an unmoved
    instance's object space.  (The child two instances of this scene share is a sphere; no box of it is shared.)"""
    idx, rec = [], []
    for i in range(len(instances)):
        child = int(instances["child"][i])
        kind, index = (child & 0xFFFFFFFF) >> 28, child & 0x0FFFFFFF
        if kind == qx.BOX:
            first = _box_first(gpu, index)
            idx += list(range(first, first + 6))
            rec.append(_resized(gpu, quads, first, (1.25, 0.8, 1.1)))
        elif kind == qx.QUAD:
            idx.append(index)
            rec.append(gpu.quad_record(quads["Q"][index] + np.float32(0.1) * quads["u"][index], quads["u"][index], quads["v"][index], int(quads["mat"][index])))
    assert len(rec) >= 4
    return np.array(idx, np.int32), np.concatenate(rec), None, None


def _box_first(gpu, index):
    return _cache["boxes"][index]


REAL = {"cornell": (32, 32, _moved_cornell, (278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0, 800.0),
        "quads": (32, 32, _moved_quads, (0.0, 0.0, 9.0), (0.0, 0.0, 0.0), 80.0, 10.0),
        "instanced": (48, 32, _moved_instanced, (-1.5, 2.5, 8.0), (-1.5, 0.5, -1.0), 64.0, 9.0)}


def _real(gpu, name, degrees):
    """An 8-spp frame and the feature buffers of the named scene as built, then -- after update_quads (and update_instances), under
    a camera `degrees` further round -- a 4-spp frame and its feature buffers; the device's own buffers and records of both
    states."""
    key = (name, degrees)
    if key not in _cache:
        nx, ny, move, eye, lookat, vfov, focus = REAL[name]
        hs = gpu.HostScene(name, nx, ny)
        built = gpu.RtCamera.from_buffer_copy(hs.desc.camera)
        cams = [built, built if degrees == 0.0 else
                gpu.make_camera(rx.orbit(eye, lookat, degrees), lookat, (0.0, 1.0, 0.0), vfov, nx / ny, 0.0, focus, 0.0, 1.0)]
        media = hs.media().copy()
        ds = gpu.DeviceScene(hs)
        try:
            _cache["boxes"] = [int(w) & 0x0FFFFFFF for w in ds.debug_quads()[1]]
            idx, rec, iidx, irec = move(gpu, ds.quads(), ds.instances())
            aov, color, records, irecords = [], [], [], []
            for k, (cam, ns) in enumerate(zip(cams, (8, 4))):
                if k:
                    ds.update_quads(rec, idx)
                    if iidx is not None:
                        ds.update_instances(irec, iidx)
                ds.set_camera(cam)
                records.append(ds.quads())
                irecords.append(ds.instances())
                color.append(ds.render(hs.frame(nx=nx, ny=ny, ns=ns, gamma=1.0))[0])
                aov.append(ds.render_aov(hs.frame(nx=nx, ny=ny, ns=4, gamma=1.0), albedo=False, ids=True))
        finally:
            ds.close()
            hs.close()
        kw = dict(color=color[1], depth=aov[1]["depth"], alpha=aov[1]["alpha"], normal=aov[1]["normal"], prim=aov[1]["prim"], inst=aov[1]["inst"],
                  history=color[0], history_len=np.ones((ny, nx), np.float32), prev_depth=aov[0]["depth"], prev_alpha=aov[0]["alpha"],
                  prev_normal=aov[0]["normal"], prev_prim=aov[0]["prim"], prev_inst=aov[0]["inst"])
        tables = dict(quads=records[1], prev_quads=records[0], instances=irecords[1], prev_instances=irecords[0], media=media)
        _cache[key] = dict(cur=cams[1], prev=cams[0], kw=kw, tables=tables, idx=idx, want=qx.reproject(cur=cams[1], prev=cams[0], **kw, **tables))
    return _cache[key]


@pytest.mark.parametrize("degrees", [0.0, 4.0])
@pytest.mark.parametrize("name", ["cornell", "quads", "instanced"])
def test_real_frames_between_which_quads_moved(gpu, name, degrees):
    """cornell at 32 x 32 (the short block taller while its instance turns, the light slid), quads at 32 x 32 (one quad translated,
    one sheared) and instanced at 48 x 32 (boxes and quads under standing instances resized and slid), under a still camera and
    under a 4 degree orbit.  Beside the parity: some pixel shows a moved quad, and some of those find a history under the new
    entry -- both counts from the restatement, so a failure there is a finding about the inputs.  The count under
    rt_reproject_instances' rule is printed beside them; DESIGN.md 4.21 has the table."""
    r = _real(gpu, name, degrees)
    kw, want, t = r["kw"], r["want"], r["tables"]
    moved = np.flatnonzero(qx.quad_records_differ(t["quads"], t["prev_quads"]))
    assert len(moved) >= 2 and set(moved.tolist()) <= set(r["idx"].tolist())    # (a box's bottom face stays when it grows taller)
    surface = kw["alpha"] >= 0.5
    on_moved = qx.shows_moved(kw["prim"], kw["inst"], len(t["quads"]), len(t["instances"]), moved) & surface
    unfollowed = ix.reproject(cur=r["cur"], prev=r["prev"], **kw, **qx.without_quads(t))
    counts = (int(on_moved.sum()), int((want[1][on_moved] > 1).sum()), int((unfollowed[1][on_moved] > 1).sum()))
    print("%s, %g degrees: moved-quad pixels %d, with a history %d following and %d under rt_reproject_instances' rule" % ((name, degrees) + counts))
    assert counts[0] > 0 and counts[1] > 0, counts
    if name != "quads":
        assert (on_moved & (kw["inst"] >= 0)).any()             # carried in an instance's object space
    _check(gpu.reproject(cur=r["cur"], prev=r["prev"], motion=True, **kw, **t), want, f"{name}, {degrees} degrees")


def _words(records, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(records).view(np.int32).reshape(len(records), -1).copy()).to(dev)


def test_device_tensors_and_a_side_stream(gpu):
    """Device tensors -- buffers, planes and tables -- are used in place and give the host arrays' result: a blocking call, and a
    non-blocking one on a side stream followed by a synchronise; inputs and tables are left alone; a host pointer declared a
    device table is refused by name."""
    import torch
    r = _real(gpu, "cornell", 4.0)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in r["kw"].items()}
    tab = {k: _words(v, dev) for k, v in r["tables"].items() if len(v)}         # (the Cornell box has no medium: no table)
    assert tab["quads"].shape[1] == 20 and tab["instances"].shape[1] == 8
    got = gpu.reproject(cur=r["cur"], prev=r["prev"], motion=True, **t, **tab)
    _check(gpu.ReprojectResult(*(x.cpu().numpy() for x in got)), r["want"], "device tensors")
    ny, nx = r["want"][1].shape
    out = torch.full((ny, nx, 3), -7.0, dtype=torch.float32, device=dev)
    out_len = torch.full((ny, nx), -7.0, dtype=torch.float32, device=dev)
    motion = torch.full((ny, nx, 2), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ret = gpu.reproject(cur=r["cur"], prev=r["prev"], out=out, out_len=out_len, motion=motion, stream=side, blocking=False, **t, **tab)
    side.synchronize()
    assert ret.out is out and ret.length is out_len and ret.motion is motion
    _check(gpu.ReprojectResult(out.cpu().numpy(), out_len.cpu().numpy(), motion.cpu().numpy()), r["want"], "side stream")
    for k, v in r["kw"].items():
        assert np.array_equal(t[k].cpu().numpy().view(np.uint32), np.ascontiguousarray(v).view(np.uint32)), k
    for k, v in tab.items():
        assert v.cpu().numpy().tobytes() == np.ascontiguousarray(r["tables"][k]).tobytes(), k
    with pytest.raises(ValueError):
        gpu.reproject(cur=r["cur"], prev=r["prev"], **t, **dict(tab, quads=r["tables"]["quads"]))      # mixed kinds
    with pytest.raises(ValueError):
        gpu.reproject(cur=r["cur"], prev=r["prev"], **t, **dict(tab, prev_quads=tab["quads"][:-1].contiguous()))
    d, m, im, qm = gpu.RtReprojectDesc(), gpu.RtReprojectMotionDesc(), gpu.RtReprojectInstanceDesc(), gpu.RtReprojectQuadDesc()
    d.nx, d.ny, d.cur, d.prev = nx, ny, r["cur"], r["prev"]
    d.color, d.depth, d.alpha, d.out, d.out_len = (x.data_ptr() for x in (t["color"], t["depth"], t["alpha"], out, out_len))
    d.prim, d.prev_prim = t["prim"].data_ptr(), t["prev_prim"].data_ptr()
    d.alpha_min, d.depth_tol, d.normal_min, d.max_history = 0.5, 0.05, 0.5, 32.0
    im.inst = t["inst"].data_ptr()
    host_table = np.ascontiguousarray(r["tables"]["prev_quads"])
    qm.n_quads, qm.quads, qm.prev_quads = len(host_table), tab["quads"].data_ptr(), host_table.ctypes.data   # host memory, declared device memory
    L = gpu.rt_lib()
    assert L.rt_reproject_quads(C.byref(d), C.byref(m), C.byref(im), C.byref(qm), 1, None, 1) == 1
    text = L.rt_last_error_detail().decode()
    assert text.startswith("rt_reproject_quads") and "prev_quads" in text and "device memory" in text, text


def test_temporal_accumulator_follows_quads(gpu):
    """push() over three cameras with two updates -- the short block taller, then its instance turned as well and the light slid --
    against update_quads, update_instances, set_camera, render, render_aov and reproject(quads=...) called by hand, and the
    restatement.  With follow_quads=False the same pushes, the updates made on the scene directly, are the plain accumulator:
    rt_reproject of the same buffers.  The flag changes the history lengths on the moved-quad pixels."""
    nx, ny, ns = 32, 32, 4
    hs = gpu.HostScene("cornell", nx, ny)
    eye, lookat = (278.0, 278.0, -800.0), (278.0, 278.0, 0.0)
    cams = [hs.desc.camera] + [gpu.make_camera(rx.orbit(eye, lookat, d), lookat, (0.0, 1.0, 0.0), 40.0, nx / ny, 0.0, 800.0, 0.0, 1.0) for d in (3.0, 6.0)]
    frame, f1 = hs.frame(nx=nx, ny=ny, ns=ns, gamma=2.0), hs.frame(nx=nx, ny=ny, ns=ns, gamma=1.0)
    base, base_i = hs.quads().copy(), hs.instances().copy()
    idx, rec, iidx, irec = _moved_cornell(gpu, base, base_i)
    updates = [None, (_resized(gpu, base, 3, (1.0, 1.2, 1.0)), None, 3), (rec, idx, 0)]
    media = hs.media()

    def by_hand(ds, follow):
        prev, result = None, []
        for k, (c, u) in enumerate(zip(cams, updates)):
            if u is not None:
                ds.update_quads(*u)
            if k == 2:
                ds.update_instances(irec, iidx)
            records, irecords = ds.quads(), ds.instances()
            ds.set_camera(c)
            color, _ = ds.render(f1)
            a = ds.render_aov(f1, albedo=False, ids=True)
            kw = dict(color=color, depth=a["depth"], alpha=a["alpha"])
            if prev is None:
                r = gpu.reproject(cur=c, prev=c, depth_tol=0.1, **kw)
            else:
                kw.update(normal=a["normal"], prim=a["prim"], history=prev["out"], history_len=prev["len"], prev_depth=prev["a"]["depth"],
                          prev_alpha=prev["a"]["alpha"], prev_normal=prev["a"]["normal"], prev_prim=prev["a"]["prim"])
                if follow:
                    more = dict(quads=records, prev_quads=prev["records"], instances=irecords, prev_instances=prev["irecords"], media=media,
                                inst=a["inst"], prev_inst=prev["a"]["inst"])
                    r = gpu.reproject(cur=c, prev=prev["cam"], depth_tol=0.1, **kw, **more)
                    _check(r, qx.reproject(cur=c, prev=prev["cam"], depth_tol=0.1, **kw, **more), "by hand, following", motion=False)
                else:
                    r = gpu.reproject(cur=c, prev=prev["cam"], depth_tol=0.1, **kw)
                    _check(r, rx.reproject(cur=c, prev=prev["cam"], depth_tol=0.1, **kw), "by hand, static", motion=False)
            prev = dict(out=r.out, len=r.length, a=a, cam=c, records=records, irecords=irecords)
            result.append((r.out, r.length, a["prim"], a["inst"]))
        return result

    def restore(ds):
        ds.update_quads(base)
        ds.update_instances(base_i)

    ds = gpu.DeviceScene(hs)
    try:
        acc = gpu.TemporalAccumulator(ds, frame, depth_tol=0.1, follow_quads=True)
        pushed = []
        for k, (c, u) in enumerate(zip(cams, updates)):
            if k == 2:
                ds.update_instances(irec, iidx)          # an update the caller made on the scene is followed just the same
            out = acc.push(c) if u is None else acc.push(c, quads=u[0], quad_indices=u[1], quad_first=u[2])
            pushed.append((out.copy(), acc.length.copy()))
        assert not qx.quad_records_differ(ds.quads()[idx], rec).any() and qx.quad_records_differ(rec, base[idx]).sum() == len(idx) - 1
        restore(ds)
        hand = by_hand(ds, True)
        restore(ds)
        plain = gpu.TemporalAccumulator(ds, frame, depth_tol=0.1)
        unfollowed = []
        for k, (c, u) in enumerate(zip(cams, updates)):
            if u is not None:
                ds.update_quads(*u)
            if k == 2:
                ds.update_instances(irec, iidx)
            unfollowed.append((plain.push(c).copy(), plain.length.copy()))
        with pytest.raises(ValueError):
            plain.push(cams[0], quads=updates[1][0])
        restore(ds)
        static = by_hand(ds, False)
    finally:
        ds.close()
        hs.close()
    for k in range(3):
        _assert_same(pushed[k][0], hand[k][0], f"push {k} out")
        _assert_same(pushed[k][1], hand[k][1], f"push {k} length")
        _assert_same(unfollowed[k][0], static[k][0], f"unfollowed push {k} out")
        _assert_same(unfollowed[k][1], static[k][1], f"unfollowed push {k} length")
    assert (pushed[0][1] == 1).all() and (pushed[2][1] == 3).any() and (pushed[2][1] == 1).any()
    for k in (1, 2):                                            # the flag changes the output on the moved-quad pixels
        moved = np.arange(3, 9) if k == 1 else idx
        on_moved = qx.shows_moved(hand[k][2], hand[k][3], len(base), len(base_i), moved)
        assert on_moved.any() and not np.array_equal(pushed[k][1][on_moved], unfollowed[k][1][on_moved]), k
        assert not np.array_equal(pushed[k][0][on_moved], unfollowed[k][0][on_moved]), k
