"""rt_render_adaptive / DeviceScene.render_adaptive on the GPU: every pixel, its sample count and the ray total equal what the
CPU oracle predicts (tests/adaptive_expect.py) bit for bit; the two identities with rt_render; gamma; a row-partitioned share;
the routes; device outputs; no clobbered scene state; the CLI."""
import os
import subprocess

import numpy as np
import pytest

import adaptive_expect as ax

pytestmark = pytest.mark.gpu

NX, NY = 32, 24
MIN, MAX = 4, 32
FLOOR = 0.01
SCENES = ["bouncing", "cornell", "cornell_smoke", "earth", "perlin", "final", "instanced", "fog", "crowd_2400", "crowd_4097",
          "crowd_big", "degenerate"]


@pytest.fixture(scope="module")
def scenes(gpu, orc):
    cache = {}

    def get(name, nx=NX, ny=NY):
        key = (name, nx, ny)
        if key not in cache:
            img, iw, ih = gpu.default_texture(name)
            hs = gpu.HostScene(name, nx, ny, img, iw, ih)
            ex = ax.Expectation(orc.OracleScene(name, nx, ny, img, iw, ih))
            cache[key] = (hs, gpu.DeviceScene(hs), ex)
        return cache[key]
    yield get
    for _, ds, _ in cache.values():
        ds.close()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _check_frame(fb, spp, st, ex, min_spp, max_spp, t, gamma):
    efb, espp, erays, esamples = ex.predict(min_spp, max_spp, t, FLOOR, gamma)
    assert np.array_equal(spp, espp), int((spp != espp).sum())
    bad = _bits(fb) != _bits(efb)
    assert not bad.any(), (int(bad.any(axis=-1).sum()), float(np.nanmax(np.abs(fb - efb))))
    assert st.rays == int(erays.sum()), (st.rays, int(erays.sum()))
    assert st.samples == int(esamples.sum())
    return espp


@pytest.mark.parametrize("name", SCENES)
def test_frame_matches_oracle(scenes, name):
    hs, ds, ex = scenes(name)
    t = ex.threshold_with_spread(MIN, MAX, FLOOR)
    assert t is not None, "no candidate threshold gives three distinct counts"
    fb, spp, st = ds.render_adaptive(hs.frame(ns=1), MIN, MAX, t, FLOOR)
    espp = _check_frame(fb, spp, st, ex, MIN, MAX, t, hs.gamma)
    assert len(np.unique(espp)) >= 3
    assert st.local_rows == NY and st.reserved >= 3


@pytest.mark.parametrize("name", ["bouncing", "cornell_smoke", "final"])
def test_identities_with_rt_render(scenes, name):
    hs, ds, ex = scenes(name)
    # threshold < 0: every pixel runs to max_spp -- the frame of rt_render at ns = max_spp
    fb, spp, st = ds.render_adaptive(hs.frame(ns=7), MIN, MAX, -1.0, FLOOR)
    ref, rst = ds.render(hs.frame(ns=MAX))
    assert (spp == MAX).all()
    assert np.array_equal(_bits(fb), _bits(ref)) and st.rays == rst.rays and st.samples == rst.samples
    # K = 0: every pixel stops at min_spp -- the frame of rt_render at ns = min_spp
    fb, spp, st = ds.render_adaptive(hs.frame(ns=7), 6, 6, 0.0, FLOOR)
    ref, rst = ds.render(hs.frame(ns=6))
    assert (spp == 6).all()
    assert np.array_equal(_bits(fb), _bits(ref)) and st.rays == rst.rays and st.samples == rst.samples


def test_gamma(scenes):
    hs, ds, ex = scenes("bouncing")
    t = ex.threshold_with_spread(MIN, MAX, FLOOR)
    fb1, spp1, _ = ds.render_adaptive(hs.frame(ns=1, gamma=1.0), MIN, MAX, t, FLOOR)
    fb2, spp2, st2 = ds.render_adaptive(hs.frame(ns=1, gamma=2.2), MIN, MAX, t, FLOOR)
    assert np.array_equal(spp1, spp2)
    _check_frame(fb2, spp2, st2, ex, MIN, MAX, t, 2.2)
    assert not np.array_equal(_bits(fb1), _bits(fb2))


@pytest.mark.parametrize("name", ["bouncing", "cornell"])
def test_row_partition(gpu, scenes, name):
    """4-row tiles dealt to a world of 3: each share equals the matching rows of the whole frame."""
    hs, ds, ex = scenes(name)
    t = ex.threshold_with_spread(MIN, MAX, FLOOR)
    whole, wspp, wst = ds.render_adaptive(hs.frame(ns=1), MIN, MAX, t, FLOOR)
    rays = samples = 0
    for rank in range(3):
        f = hs.frame(ns=1, tile_rows=4, tile_first=rank, tile_stride=3)
        rows = gpu.local_rows_to_global(f)
        fb, spp, st = ds.render_adaptive(f, MIN, MAX, t, FLOOR)
        assert fb.shape == (len(rows), NX, 3) and st.local_rows == len(rows)
        assert np.array_equal(_bits(fb), _bits(whole[rows])) and np.array_equal(spp, wspp[rows])
        rays += st.rays
        samples += st.samples
    assert rays == wst.rays and samples == wst.samples


@pytest.mark.parametrize("name", ["bouncing", "cornell", "crowd_2400", "crowd_big"])
def test_routes_change_nothing(gpu, scenes, name):
    hs, ds, ex = scenes(name)
    t = ex.threshold_with_spread(MIN, MAX, FLOOR)
    got = {}
    for route in (0, 1, -1):
        gpu.set_option("adaptive_tier", route)
        fb, spp, st = ds.render_adaptive(hs.frame(ns=1), MIN, MAX, t, FLOOR)
        passes = ds.adaptive_passes()
        got[route] = (fb, spp, st.rays, st.samples, [p["route"] for p in passes])
        assert len(passes) == st.reserved and all(p["active"] > 0 for p in passes)
    gpu.reset_options()
    for route in (1, -1):
        assert np.array_equal(_bits(got[route][0]), _bits(got[0][0])) and np.array_equal(got[route][1], got[0][1])
        assert got[route][2:4] == got[0][2:4]
    assert set(got[0][4]) == {"main"}
    list_passes = got[1][4][2:]
    assert list_passes, "no pass over an active list"
    if name == "crowd_big":   # more than 4 096 leaves: no tier data, the forced route falls back to the main kernel
        assert set(got[1][4]) == {"main"}
    else:
        assert set(list_passes) == {"tier"}
    _check_frame(got[1][0], got[1][1], type("S", (), {"rays": got[1][2], "samples": got[1][3]}), ex, MIN, MAX, t, hs.gamma)


def test_device_outputs(gpu, scenes):
    import torch
    hs, ds, ex = scenes("cornell")
    t = ex.threshold_with_spread(MIN, MAX, FLOOR)
    fb, spp, st = ds.render_adaptive(hs.frame(ns=1), MIN, MAX, t, FLOOR)
    out = torch.full((NY, NX, 3), float("nan"), dtype=torch.float32, device="cuda:0")
    sppd = torch.full((NY, NX), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    r_fb, r_spp, st2 = ds.render_adaptive(hs.frame(ns=1), MIN, MAX, t, FLOOR, out=out, spp_out=sppd)
    assert r_fb is out and r_spp is sppd
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(fb)) and np.array_equal(sppd.cpu().numpy(), spp)
    assert st2.rays == st.rays and st2.samples == st.samples
    # no map asked for: the frame alone
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    ds.render_adaptive(hs.frame(ns=1), MIN, MAX, t, FLOOR, out=out)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(fb))
    with pytest.raises(ValueError):
        ds.render_adaptive(hs.frame(ns=1), MIN, MAX, t, FLOOR, out=out, spp_out=np.zeros((NY, NX), np.int32))


def test_render_and_trace_unchanged_after_an_adaptive_frame(scenes):
    hs, ds, ex = scenes("final")
    rng = np.random.default_rng(5)
    o = rng.uniform(-5, 5, (512, 3)).astype(np.float32)
    d = rng.standard_normal((512, 3)).astype(np.float32)
    before_fb, before_st = ds.render(hs.frame(ns=40))
    before_tr = ds.trace(o, d)
    ds.render_adaptive(hs.frame(ns=1), MIN, 64, 0.05, FLOOR)
    after_fb, after_st = ds.render(hs.frame(ns=40))
    after_tr = ds.trace(o, d)
    assert np.array_equal(_bits(before_fb), _bits(after_fb)) and before_st.rays == after_st.rays
    for x, y in zip(before_tr, after_tr):
        if x is not None:
            assert np.array_equal(x, y)


def test_cli_prints_the_python_result(gpu, scenes, tmp_path):
    nx, ny, ns, t = 40, 30, 64, 0.1
    hs, ds, _ = scenes("bouncing", nx, ny)
    exe = os.path.join(gpu.PKG_DIR, "lib", "rayTracer")
    r = subprocess.run([exe, "--scene", "bouncing", "--nx", str(nx), "--ny", str(ny), "--ns", str(ns), "--adaptive", str(t)],
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    fb, spp, st = ds.render_adaptive(hs.frame(ns=ns), 16, ns, t, 0.01)   # default --min-spp: 16 for --ns 64
    assert len(np.unique(spp)) >= 2
    path = tmp_path / "py.ppm"
    gpu.write_ppm(str(path), fb, hs.ppm_double_scale)
    assert r.stdout == path.read_bytes()
    bad = subprocess.run([exe, "--scene", "bouncing", "--adaptive", "0.1", "--progressive", "4"], capture_output=True, timeout=60)
    assert bad.returncode == 2 and b"--adaptive" in bad.stderr
