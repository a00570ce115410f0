"""rt_reproject_instances / reproject(instances=...) / TemporalAccumulator(follow_instances=True) on the GPU.  Every comparison is
bit for bit against the NumPy restatement of the extended contract (tests/reproject_instances_expect.py), NaNs compared as equal:
out, out_len and motion, on seeded synthetic buffers whose ids, inst planes and tables reach every branch of both follow steps, at
a size that is no multiple of the tile, on small frames, on the identities with rt_reproject_moving and rt_reproject, on real
pairs of frames between which instances moved, from host arrays and device tensors, on a side stream, and through the
accumulator."""
import ctypes as C

import numpy as np
import pytest

import reproject_expect as rx
import reproject_instances_expect as ix
import reproject_moving_expect as mx

pytestmark = pytest.mark.gpu

NX, NY = 37, 29            # three tiles by two, neither a multiple of 16
TIGHT = dict(alpha_min=0.75, depth_tol=0.0, normal_min=0.9, max_history=4.0)
_cache = {}


def _synthetic():
    if "synthetic" not in _cache:
        _cache["synthetic"] = ix.synthetic_instances(NX, NY, 7)
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
def test_synthetic_buffers_every_branch_of_both_follow_steps(gpu, normals, motion):
    """The inputs tests/test_reproject_instances_host.py counts the branches of, under a previous camera a few degrees away, the
    same camera, and one the points are behind (a <= 0); then the tight thresholds, the ranges' ends among them."""
    s = _synthetic()
    kw, t = ix.select(s["buffers"], normals), s["tables"]
    for name, prev in s["cams"].items():
        want = ix.reproject(cur=s["cur"], prev=prev, **kw, **t)
        got = gpu.reproject(cur=s["cur"], prev=prev, motion=motion, **kw, **t)
        _check(got, want, f"{name} normals={normals}", motion)
        want = ix.reproject(cur=s["cur"], prev=prev, **kw, **t, **TIGHT)
        _check(gpu.reproject(cur=s["cur"], prev=prev, motion=motion, **kw, **t, **TIGHT), want, f"{name} tight thresholds", motion)


@pytest.mark.parametrize("nx,ny", [(1, 1), (16, 16), (17, 1), (1, 33)])
def test_small_and_tile_sized_frames(gpu, nx, ny):
    s = ix.synthetic_instances(nx, ny, 100 * nx + ny)
    for prev in s["cams"].values():
        _check(gpu.reproject(cur=s["cur"], prev=prev, motion=True, **s["buffers"], **s["tables"]),
               ix.reproject(cur=s["cur"], prev=prev, **s["buffers"], **s["tables"]), f"{nx}x{ny}")


def test_identities_with_the_other_two_entries(gpu):
    """n_instances = 0 (null tables, through the binding and through the C entry with a description of zeros) against
    rt_reproject_moving with the moving sphere tables, and unmoved instance tables without sphere tables against rt_reproject: the
    device's own bits of the same buffers for every camera, with inst = -1 everywhere -- and on the painted planes the new
    entry's result with no table is rt_reproject_moving's wherever the tap test on inst cannot bite.  A null history: out ==
    color and out_len == 1, with the followed motion still written."""
    s = _synthetic()
    t = s["tables"]
    none = np.full((NY, NX), -1, np.int32)
    b = dict(s["buffers"], inst=none, prev_inst=none)
    plain = ix.without_inst(b)
    spheres = {k: t[k] for k in ("spheres", "prev_spheres", "media", "time", "prev_time")}
    cur, same, media = ix.unmoved_instance_tables()
    empty = np.zeros(0, gpu.INSTANCE_DTYPE)
    L = gpu.rt_lib()
    for name, prev in s["cams"].items():
        moving = tuple(np.ascontiguousarray(x) for x in gpu.reproject(cur=s["cur"], prev=prev, motion=True, **plain, **spheres))
        _check(gpu.reproject(cur=s["cur"], prev=prev, motion=True, instances=empty, prev_instances=empty, **b, **spheres), moving, f"{name} empty tables")
        static = tuple(np.ascontiguousarray(x) for x in gpu.reproject(cur=s["cur"], prev=prev, motion=True, **plain))
        _check(gpu.reproject(cur=s["cur"], prev=prev, motion=True, instances=cur, prev_instances=same, media=media, **b), static, f"{name} unmoved tables")
        # the C entry itself with descriptions of nothing but zeros and the two planes
        d, m, im = gpu.RtReprojectDesc(), gpu.RtReprojectMotionDesc(), gpu.RtReprojectInstanceDesc()
        d.nx, d.ny, d.cur, d.prev = NX, NY, s["cur"], prev
        out, out_len, mot = np.full((NY, NX, 3), -7, np.float32), np.full((NY, NX), -7, np.float32), np.full((NY, NX, 2), -7, np.float32)
        for k, v in dict(plain, out=out, out_len=out_len, motion=mot).items():
            setattr(d, k, v.ctypes.data)
        d.alpha_min, d.depth_tol, d.normal_min, d.max_history = (rx.DEFAULTS[k] for k in ("alpha_min", "depth_tol", "normal_min", "max_history"))
        im.inst, im.prev_inst = none.ctypes.data, none.ctypes.data
        assert L.rt_reproject_instances(C.byref(d), C.byref(m), C.byref(im), 0, None, 1) == 0, L.rt_last_error_detail().decode()
        _check(gpu.ReprojectResult(out, out_len, mot), static, f"{name} n_instances = 0, n_spheres = 0")
    p = s["buffers"]
    first = gpu.reproject(p["color"], p["depth"], p["alpha"], s["cur"], s["cams"]["near"], normal=p["normal"], prim=p["prim"],
                          prev_normal=p["prev_normal"], prev_prim=p["prev_prim"], inst=p["inst"], motion=True, **t)
    assert np.array_equal(first.out.view(np.uint32), p["color"].view(np.uint32))
    assert np.array_equal(first.length, np.ones((NY, NX), np.float32))
    _assert_same(first.motion, ix.reproject(cur=s["cur"], prev=s["cams"]["near"], **p, **t)[2], "first frame motion")
    unfollowed = gpu.reproject(p["color"], p["depth"], p["alpha"], s["cur"], s["cams"]["near"], prim=p["prim"], prev_prim=p["prev_prim"],
                               motion=True, **spheres)
    assert not np.array_equal(first.motion, unfollowed.motion, equal_nan=True)


# --------------------------------------------------------------------------------------------------------- real pairs
def _moved_cornell_smoke(records):
    """Both instances (each bounds a medium) turned by 6 degrees."""
    return np.arange(len(records)), ix.turned(records, np.arange(len(records)), 6.0)


def _moved_instanced(records):
    """The two instances that share a child moved differently -- one shifted, one shifted the other way and turned by 25 degrees
    -- and, so that more than a few pixels take the path, every box under translate(rotate_y(.)) turned by 9 degrees."""
    child = records["child"]
    shared = [i for i in range(len(records)) if (child == child[i]).sum() == 2]
    assert len(shared) == 2
    boxes = [i for i in range(len(records)) if records["flags"][i] == 3 and (int(child[i]) >> 28) == ix.BOX and i not in shared]
    assert boxes
    idx = np.array(shared + boxes)
    rec = np.concatenate([ix.turned(records, shared[:1], 0.0, (0.3, 0.0, 0.0)), ix.turned(records, shared[1:], 25.0, (-0.25, 0.0, 0.2)),
                          ix.turned(records, boxes, 9.0)])
    return idx, rec


REAL = {"cornell_smoke": (32, 32, _moved_cornell_smoke, (278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0, 800.0),
        "instanced": (48, 32, _moved_instanced, (-1.5, 2.5, 8.0), (-1.5, 0.5, -1.0), 64.0, 9.0)}


def _real(gpu, name, degrees):
    """An 8-spp frame and the feature buffers of the named scene as built, then -- after update_instances, under a camera
    `degrees` further round -- a 4-spp frame and its feature buffers; the device's own buffers and records of both states."""
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
            idx, rec = move(ds.instances())
            aov, color, records = [], [], []
            for k, (cam, ns) in enumerate(zip(cams, (8, 4))):
                if k:
                    ds.update_instances(rec, idx.astype(np.int32))
                ds.set_camera(cam)
                records.append(ds.instances())
                color.append(ds.render(hs.frame(nx=nx, ny=ny, ns=ns, gamma=1.0))[0])
                aov.append(ds.render_aov(hs.frame(nx=nx, ny=ny, ns=4, gamma=1.0), albedo=False, ids=True))
        finally:
            ds.close()
            hs.close()
        kw = dict(color=color[1], depth=aov[1]["depth"], alpha=aov[1]["alpha"], normal=aov[1]["normal"], prim=aov[1]["prim"], inst=aov[1]["inst"],
                  history=color[0], history_len=np.ones((ny, nx), np.float32), prev_depth=aov[0]["depth"], prev_alpha=aov[0]["alpha"],
                  prev_normal=aov[0]["normal"], prev_prim=aov[0]["prim"], prev_inst=aov[0]["inst"])
        tables = dict(instances=records[1], prev_instances=records[0], media=media)
        _cache[key] = dict(cur=cams[1], prev=cams[0], kw=kw, tables=tables, idx=idx, want=ix.reproject(cur=cams[1], prev=cams[0], **kw, **tables))
    return _cache[key]


@pytest.mark.parametrize("degrees", [0.0, 4.0])
@pytest.mark.parametrize("name", ["cornell_smoke", "instanced"])
def test_real_frames_between_which_instances_moved(gpu, name, degrees):
    """cornell_smoke at 32 x 32 (both instances bound media, both turned by 6 degrees) and instanced at 48 x 32 (the two instances
    of one child moved differently), under a still camera and under a 4 degree orbit.  Beside the parity: some pixel shows a
    moved instance, and strictly more moved-instance pixels find a history with following than rt_reproject_moving's rule finds
    on the same buffers -- both counts from the restatements, so a failure there is a finding about the inputs.  The counts the
    device's buffers gave are in DESIGN.md 4.19."""
    r = _real(gpu, name, degrees)
    kw, want, t = r["kw"], r["want"], r["tables"]
    assert not np.array_equal(t["instances"], t["prev_instances"])
    surface = kw["alpha"] >= 0.5
    on_moved = ix.shows_moved(kw["inst"], kw["prim"], t["media"], len(t["instances"]), r["idx"]) & surface
    unfollowed = mx.reproject(cur=r["cur"], prev=r["prev"], **ix.without_inst(kw), media=t["media"])
    counts = (int(on_moved.sum()), int((want[1][on_moved] > 1).sum()), int((unfollowed[1][on_moved] > 1).sum()))
    print("%s, %g degrees: moved-instance pixels %d, with a history %d following and %d not" % ((name, degrees) + counts))
    assert counts[0] > 0 and counts[1] > counts[2], counts
    if name == "instanced":     # the two instances of one child show one prim id: only inst tells their pixels apart
        shared = r["idx"][:2]
        a, b = (kw["inst"] == shared[0]), (kw["inst"] == shared[1])
        assert a.any() and b.any() and len(set(kw["prim"][a | b].tolist())) == 1
    _check(gpu.reproject(cur=r["cur"], prev=r["prev"], motion=True, **kw, **t), want, f"{name}, {degrees} degrees")


def _words(records, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(records).view(np.int32).reshape(len(records), -1).copy()).to(dev)


def test_device_tensors_and_a_side_stream(gpu):
    """Device tensors -- buffers, planes and tables -- are used in place and give the host arrays' result: a blocking call, and a
    non-blocking one on a side stream followed by a synchronise; inputs and tables are left alone; a host pointer declared a
    device table is refused by name."""
    import torch
    r = _real(gpu, "cornell_smoke", 4.0)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in r["kw"].items()}
    tab = {k: _words(v, dev) for k, v in r["tables"].items()}
    assert tab["instances"].shape[1] == 8 and tab["media"].shape[1] == 4
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
    for k, v in r["tables"].items():
        assert tab[k].cpu().numpy().tobytes() == np.ascontiguousarray(v).tobytes(), k
    with pytest.raises(ValueError):
        gpu.reproject(cur=r["cur"], prev=r["prev"], **t, **dict(tab, instances=r["tables"]["instances"]))      # mixed kinds
    with pytest.raises(ValueError):
        gpu.reproject(cur=r["cur"], prev=r["prev"], **t, **dict(tab, prev_instances=tab["instances"][:-1].contiguous()))
    d, m, im = gpu.RtReprojectDesc(), gpu.RtReprojectMotionDesc(), gpu.RtReprojectInstanceDesc()
    d.nx, d.ny, d.cur, d.prev = nx, ny, r["cur"], r["prev"]
    d.color, d.depth, d.alpha, d.out, d.out_len = (x.data_ptr() for x in (t["color"], t["depth"], t["alpha"], out, out_len))
    d.prim, d.prev_prim = t["prim"].data_ptr(), t["prev_prim"].data_ptr()
    d.alpha_min, d.depth_tol, d.normal_min, d.max_history = 0.5, 0.05, 0.5, 32.0
    host_table = np.ascontiguousarray(r["tables"]["prev_instances"])
    im.n_instances, im.instances, im.prev_instances = len(host_table), tab["instances"].data_ptr(), host_table.ctypes.data   # host memory, declared device memory
    im.inst = t["inst"].data_ptr()
    L = gpu.rt_lib()
    assert L.rt_reproject_instances(C.byref(d), C.byref(m), C.byref(im), 1, None, 1) == 1
    text = L.rt_last_error_detail().decode()
    assert text.startswith("rt_reproject_instances") and "prev_instances" in text and "device memory" in text, text


def test_temporal_accumulator_follows_instances(gpu):
    """push() over three cameras with two updates against update_instances, set_camera, render, render_aov and
    reproject(instances=...) called by hand -- and the restatement.  With follow_instances=False the same pushes, the updates made
    on the scene directly, are today's accumulator: rt_reproject of the same buffers.  Passing the update without the flag is a
    ValueError."""
    nx, ny, ns = 32, 32, 4
    hs = gpu.HostScene("cornell_smoke", nx, ny)
    eye, lookat = (278.0, 278.0, -800.0), (278.0, 278.0, 0.0)
    cams = [hs.desc.camera] + [gpu.make_camera(rx.orbit(eye, lookat, d), lookat, (0.0, 1.0, 0.0), 40.0, nx / ny, 0.0, 800.0, 0.0, 1.0) for d in (3.0, 6.0)]
    frame, f1 = hs.frame(nx=nx, ny=ny, ns=ns, gamma=2.0), hs.frame(nx=nx, ny=ny, ns=ns, gamma=1.0)
    base = hs.instances()
    updates = [None, (ix.turned(base, [0, 1], 6.0), None), (ix.turned(base, [1], -9.0, (4.0, 0.0, -3.0)), np.array([1], np.int32))]
    media = hs.media()

    def by_hand(ds, follow):
        prev, result = None, []
        for c, u in zip(cams, updates):
            if u is not None:
                ds.update_instances(*u)
            records = ds.instances()
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
                    more = dict(instances=records, prev_instances=prev["records"], media=media, inst=a["inst"], prev_inst=prev["a"]["inst"])
                    r = gpu.reproject(cur=c, prev=prev["cam"], depth_tol=0.1, **kw, **more)
                    _check(r, ix.reproject(cur=c, prev=prev["cam"], depth_tol=0.1, **kw, **more), "by hand, following", motion=False)
                else:
                    r = gpu.reproject(cur=c, prev=prev["cam"], depth_tol=0.1, **kw)
                    _check(r, rx.reproject(cur=c, prev=prev["cam"], depth_tol=0.1, **kw), "by hand, static", motion=False)
            prev = dict(out=r.out, len=r.length, a=a, cam=c, records=records)
            result.append((r.out, r.length))
        return result

    ds = gpu.DeviceScene(hs)
    try:
        acc = gpu.TemporalAccumulator(ds, frame, depth_tol=0.1, follow_instances=True)
        pushed = []
        for c, u in zip(cams, updates):
            out = acc.push(c) if u is None else acc.push(c, instances=u[0], instance_indices=u[1])
            pushed.append((out.copy(), acc.length.copy()))
        ds.update_instances(base)
        hand = by_hand(ds, True)
        ds.update_instances(base)
        plain = gpu.TemporalAccumulator(ds, frame, depth_tol=0.1)
        unfollowed = []
        for c, u in zip(cams, updates):
            if u is not None:
                ds.update_instances(*u)
            unfollowed.append((plain.push(c).copy(), plain.length.copy()))
        with pytest.raises(ValueError):
            plain.push(cams[0], instances=updates[1][0])
        with pytest.raises(ValueError):
            plain.push(cams[0], instance_first=1)
        ds.update_instances(base)
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
    assert not np.array_equal(pushed[1][1], unfollowed[1][1])                # following found other histories
