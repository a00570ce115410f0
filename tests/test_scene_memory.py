"""Device memory over the life of a scene (struct rt_scene and rt_progressive, csrc/rt_host.h; the owning buffers of
csrc/rt_owned.h): a scene that has allocated everything a scene can allocate gives all of it back when it is destroyed.

One cycle creates a DeviceScene, makes every cached buffer of the scene exist -- a ranked frame (parts, tiers, tail hand-off,
cost map), a second frame size, an adaptive and a variance frame (the second regrows what the first allocated), a progressive
window pair, a sphere update with recalibrate=True (the calibration prior changes hands) -- and closes everything.  After one
warm-up cycle, three more cycles must not cost more free device memory than they cost the parent commit, whose free list was
written out by hand.  A correct free list leaks nothing per cycle: the allowance is what the runtime itself retained there.

What it can see: free device memory moves in steps of 2 MiB.  A scene destroy that forgets the heavy list (2 MiB) costs 6 MiB
over the three cycles on either scene; one that forgets the calibration prior and the parked pixels (about 0.4 MiB a cycle)
cost 2 MiB on bouncing and nothing on fog.  Every buffer freeing itself is tests/owned_check.cpp's to show."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# bytes of free device memory (torch.cuda.mem_get_info) that three cycles cost the parent commit, measured by this file on a
# build of the parent, twice on an MI355X (the test prints its figure before it asserts):
#   RT_LIB_OVERRIDE=<the parent's librt_mi355x.so> python -m pytest tests/test_scene_memory.py -m gpu -s
# It kept nothing: the allowance is 0, and no margin is added to it.
PARENT_DROP_BYTES = {"bouncing": 0, "fog": 0}
CYCLES = 3


def _cycle(art, hs):
    ds = art.DeviceScene(hs)
    try:
        ds.render(hs.frame(nx=64, ny=64, ns=32))                 # the smallest ranked frame: 64 tiles, 2 x split_samples
        ds.render(hs.frame(nx=72, ny=40, ns=32))
        ds.render_adaptive(hs.frame(nx=72, ny=40), 2, 8, 0.05)
        ds.render_variance(hs.frame(nx=64, ny=64, ns=4), 2)      # more pixels than the adaptive frame parked
        win = ds.progressive(hs.frame(nx=64, ny=64, ns=4))
        try:
            win.render(0, 2)
            win.render(2, 4)
        finally:
            win.close()
        ds.update_spheres(hs.spheres()[1:2], np.array([1], np.int32), recalibrate=True)
    finally:
        ds.close()


@pytest.mark.parametrize("name", list(PARENT_DROP_BYTES))
def test_cycles_give_their_memory_back(gpu, name):
    import torch
    hs = gpu.HostScene(name, 64, 64)     # bouncing: the lean spheres-only family; fog: the general family with media and an instance

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    _cycle(gpu, hs)
    before = free_bytes()
    for _ in range(CYCLES):
        _cycle(gpu, hs)
    drop = before - free_bytes()
    print(f"{name}: {CYCLES} cycles cost {drop} bytes of free device memory (parent: {PARENT_DROP_BYTES[name]})")
    assert drop <= PARENT_DROP_BYTES[name]
