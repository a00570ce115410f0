"""Host reference of the device-side ranking and the cost prior (csrc/rt_rank.hip), for tests/test_rank_host.py and tests/test_rank.py.

Written from the comments of rt_rank.hip and DESIGN.md 4.3, not from its statements.  Every scalar integer is a Python int and
every double a Python float (binary64); the three factors are numpy.float32 widened to float, as the kernels widen them.  Arrays
with one entry per pixel or tile are numpy int64, whose arithmetic is as exact as int's in the ranges used here (a cost is below
2^31, a product with a percentage below 2^38).  The library is built with -ffp-contract=off -fno-fast-math, so a double expression
written in the kernels' order -- (double)total / n_pixels, mean * (double)factor + 0.999, the bucket midpoint, the running
`work` -- has one value: the reference expects equality, not closeness.

What the kernels leave free is never compared: the order of items inside one of the 2048 buckets of a sort, and the raw list the
collect kernel appends to (both are the order the LDS / global atomics happen to give).  check_rank_outputs() holds the assertions
that are free of it, and is run on the reference's own outputs and on the device's alike.
"""
import numpy as np

BUCKETS = 2048               # linear cost buckets of both sorts; bucket 0 holds the dearest items
TIER_WAVES_PER_WG = 4        # a tier workgroup is four waves, each with one pixel at a time
FLAG, MASK = 0x80000000, 0x7FFFFFFF
NO_LIST = 0xFFFFFFFF         # heavy_threshold when there is no list; heavy_pixels entries the ranking did not write (the seam's fill)

# the 20 words of rt_debug_rank's `params`, in the header's order
PARAM_WORDS = ("n_pixels", "n_tiles", "heavy_cap", "max_grid", "waves_per_wg", "normal_need",
               "sparse_stride", "semi_stride", "sparse_percent", "sparse_work_percent", "tier_possible", "tier1_pixels",
               "tier1_depth", "tier_wgs_cap", "tier_waves_per_main_wg", "nx", "smooth_percent",
               "heavy_factor", "sparse_factor", "tier1_factor")
# the 13 words of rt_rank_info
INFO_WORDS = ("heavy_items", "heavy_threshold", "tier1_items", "tier2_items", "tier1_wgs", "main_skip_wgs", "sparse_wgs",
              "sparse_stride", "semi_wgs", "semi_stride", "threshold1", "threshold2", "collected")
# the branch outcomes rank_info() reports (tests/test_rank_host.py asserts that the cases of rank_cases() reach every one)
OUTCOMES = ("usable", "not usable", "admission cut", "admission whole", "tier1 capped by pixels", "tier1 capped by workgroups",
            "tier1 uncapped", "sparse capped", "semi capped", "skip clamped", "list dropped by the final rule")


def pack_params(p: dict) -> np.ndarray:
    """The parameter dict as rt_debug_rank's 20 words."""
    w = np.zeros(20, np.uint32)
    for k, name in enumerate(PARAM_WORDS):
        if k < 6:
            w[k] = p[name]
        elif k < 17:
            w[k:k + 1].view(np.int32)[0] = p[name]
        else:
            w[k:k + 1].view(np.float32)[0] = np.float32(p[name])
    return w


def thresholds(total: int, n_pixels: int, factors, sparse_stride: int):
    """(heavy_threshold, threshold1, threshold2) from the mean cost per pixel; factors = (heavy, sparse, tier1) as float32.
    threshold1 goes with the tier-1 factor, threshold2 with the sparse factor; without sparse waves there is no heavy threshold."""
    heavy_f, sparse_f, tier1_f = (float(np.float32(f)) for f in factors)
    mean = float(total) / float(n_pixels)
    t1 = int(mean * tier1_f + 0.999)
    t2 = int(mean * sparse_f + 0.999)
    heavy = int(mean * heavy_f + 0.999) if sparse_stride > 0 else NO_LIST
    return heavy, t1, t2


def estimates(cost, nx: int, smooth_percent: int) -> np.ndarray:
    """Per-pixel cost estimate: the pixel's own cost (low 31 bits), or smooth_percent of its dearest 4-neighbour's if that is more.
    Neighbours are those of the local row grid: left and right within the row of nx pixels, above and below within n_pixels."""
    own = np.asarray(cost, np.int64) & MASK
    n = len(own)
    if smooth_percent <= 0 or nx <= 0:
        return own
    i = np.arange(n, dtype=np.int64)
    x = i % nx
    m = np.zeros(n, np.int64)
    left = x > 0
    m[left] = own[i[left] - 1]
    right = (x + 1 < nx) & (i + 1 < n)
    m[right] = np.maximum(m[right], own[i[right] + 1])
    up = i >= nx
    m[up] = np.maximum(m[up], own[i[up] - nx])
    down = i + nx < n
    m[down] = np.maximum(m[down], own[i[down] + nx])
    return np.maximum(own, (m * smooth_percent) // 100)


def listing(cost, est, heavy_threshold: int):
    """From the estimates: the listed pixels (ascending ids), the costs with this ranking's flags in bit 31, and `collected`."""
    listed = np.asarray(est, np.int64) >= heavy_threshold
    new_cost = ((np.asarray(cost, np.int64) & MASK) | np.where(listed, FLAG, 0)).astype(np.uint32)
    return np.flatnonzero(listed), new_cost, int(listed.sum())


def bucket(k: int, lo: int, hi: int) -> int:
    """The bucket of key k in a descending sort of keys lo..hi."""
    return ((hi - k) * BUCKETS) // (hi - lo + 1)


def buckets_of(keys) -> np.ndarray:
    """bucket() of every key of an array, lo and hi being the array's own extremes."""
    keys = np.asarray(keys, np.int64)
    lo, hi = int(keys.min()), int(keys.max())
    return ((hi - keys) * BUCKETS) // (hi - lo + 1)


def cumulative_histogram(keys) -> np.ndarray:
    """hist[b] = number of keys in buckets 0..b (inclusive), 2048 entries."""
    return np.cumsum(np.bincount(buckets_of(keys), minlength=BUCKETS)[:BUCKETS])


def _ceil_div(a: int, b: int) -> int:
    return (a + b - 1) // b


def rank_info(p: dict, cost, total: int):
    """The 13 words the ranking leaves, as a dict, and the set of branch outcomes this input took (OUTCOMES)."""
    n_pixels = int(p["n_pixels"])
    heavy_t, t1, t2 = thresholds(total, n_pixels, (p["heavy_factor"], p["sparse_factor"], p["tier1_factor"]), p["sparse_stride"])
    est = estimates(cost, p["nx"], p["smooth_percent"])
    pixels, _, count = listing(cost, est, heavy_t)
    info = dict.fromkeys(INFO_WORDS, 0)
    info.update(heavy_threshold=NO_LIST, sparse_stride=1, semi_stride=1, threshold1=t1, threshold2=t2, collected=count)
    outcomes = set()
    # no list: no sparse waves, nothing collected, more than the list holds, or half the pixels and more
    usable = p["sparse_stride"] > 0 and 0 < count <= p["heavy_cap"] and 2 * count < n_pixels
    outcomes.add("usable" if usable else "not usable")
    if not usable:
        return info, outcomes
    keys = est[pixels]
    hi, lo = int(keys.max()), int(keys.min())
    span = hi - lo + 1
    hist = cumulative_histogram(keys)
    n_tier1, n_tier2 = int((keys >= t1).sum()), int((keys >= t2).sum())
    # the dearest pixels are admitted to tiers 1 and 2 while their rays so far, bucket by bucket at the bucket's midpoint, stay
    # within sparse_work_percent of all rays
    budget = float(total) * float(p["sparse_work_percent"]) / 100.0
    work, admitted, prev, cut = 0.0, 0, 0, False
    for b in range(BUCKETS):
        upto = int(hist[b])
        nb = upto - prev
        prev = upto
        if nb == 0:
            continue
        mid = float(hi) - (float(b) + 0.5) * float(span) / float(BUCKETS)
        work += float(nb) * (mid if mid > 0.0 else 0.0)
        if work > budget:
            cut = True
            break
        admitted = upto
    outcomes.add("admission cut" if cut else "admission whole")
    n_tier1, n_tier2 = min(n_tier1, admitted), min(n_tier2, admitted)
    cap_wgs = p["max_grid"] * p["sparse_percent"] // 100
    # tier 1: one pixel per wave at a time, tier1_depth of them per wave one after the other, four waves per workgroup
    tier1_items = n_tier1 if p["tier_possible"] else 0
    if tier1_items > p["tier1_pixels"]:
        tier1_items = p["tier1_pixels"]
        outcomes.add("tier1 capped by pixels")
    depth = p["tier1_depth"] if p["tier1_depth"] > 0 else 1
    tier1_wgs = _ceil_div(tier1_items, TIER_WAVES_PER_WG * depth)
    if tier1_wgs > p["tier_wgs_cap"]:
        tier1_wgs = p["tier_wgs_cap"]
        outcomes.add("tier1 capped by workgroups")
    if tier1_wgs == 0:
        tier1_items = 0
    if tier1_items > 0 and not ({"tier1 capped by pixels", "tier1 capped by workgroups"} & outcomes):
        outcomes.add("tier1 uncapped")
    # tier 2: the rest of the pixels at or above the sparse threshold, 64 / sparse_stride per wave, as many as the sparse
    # workgroups hold at once
    tier2_items = max(n_tier2 - tier1_items, 0)
    tier2_items = min(tier2_items, count - tier1_items)
    per_wg2 = p["waves_per_wg"] * (64 // p["sparse_stride"])
    sparse_wgs = _ceil_div(tier2_items, per_wg2)
    if sparse_wgs > cap_wgs:
        sparse_wgs = cap_wgs
        outcomes.add("sparse capped")
    tier2_items = min(tier2_items, sparse_wgs * per_wg2)
    # tier 3: the rest of the list, on workgroups of its own when semi_stride > 0, in what the sparse workgroups leave of the cap
    semi_wgs = 0
    if p["semi_stride"] > 0:
        per_wg3 = p["waves_per_wg"] * (64 // p["semi_stride"])
        semi_wgs = _ceil_div(count - tier1_items - tier2_items, per_wg3)
        room = max(cap_wgs - sparse_wgs, 0)
        if semi_wgs > room:
            semi_wgs = room
            outcomes.add("semi capped")
    grid = min(p["normal_need"] + sparse_wgs + semi_wgs, p["max_grid"])
    # main workgroups that leave at once to make room for the tier kernel's waves, beyond the slots the grid leaves empty
    skip = 0
    if p["tier_waves_per_main_wg"] > 0 and tier1_wgs > 0:
        slots = _ceil_div(tier1_wgs * TIER_WAVES_PER_WG, p["tier_waves_per_main_wg"])
        spare = max(p["max_grid"] - grid, 0)
        skip = max(slots - spare, 0)
        if skip + 1 > grid:              # at least one main workgroup keeps working
            skip = grid - 1 if grid > 1 else 0
            outcomes.add("skip clamped")
    # at least one ordinary workgroup, or no list
    if grid > sparse_wgs + semi_wgs:
        info.update(heavy_items=count, heavy_threshold=heavy_t, tier1_items=tier1_items, tier2_items=tier2_items, tier1_wgs=tier1_wgs,
                    main_skip_wgs=skip, sparse_wgs=sparse_wgs, sparse_stride=p["sparse_stride"], semi_wgs=semi_wgs,
                    semi_stride=p["semi_stride"] if p["semi_stride"] > 0 else 1)
    else:
        outcomes.add("list dropped by the final rule")
    return info, outcomes


def info_words(info: dict) -> list:
    return [int(info[k]) for k in INFO_WORDS]


def reference_outputs(inputs: dict) -> dict:
    """What the ranking leaves for `inputs` = {params, cost, tile_cost, total}, with both orders built by a stable host sort by
    bucket (one of the orders the device may give).  heavy_pixels is written whenever the list was sorted -- also when the final
    rule then drops it -- and keeps the seam's fill otherwise."""
    p = inputs["params"]
    info, outcomes = rank_info(p, inputs["cost"], inputs["total"])
    est = estimates(inputs["cost"], p["nx"], p["smooth_percent"])
    pixels, new_cost, _ = listing(inputs["cost"], est, thresholds(inputs["total"], p["n_pixels"], (p["heavy_factor"], p["sparse_factor"], p["tier1_factor"]),
                                                                  p["sparse_stride"])[0])
    tile_order = np.argsort(buckets_of(inputs["tile_cost"]), kind="stable").astype(np.uint32)
    heavy_pixels = np.full(p["heavy_cap"], NO_LIST, np.uint32)
    if "usable" in outcomes:
        heavy_pixels[:len(pixels)] = pixels[np.argsort(buckets_of(est[pixels]), kind="stable")]
    return {"tile_order": tile_order, "cost_out": new_cost, "heavy_pixels": heavy_pixels, "info": info_words(info), "outcomes": outcomes}


def check_rank_outputs(inputs: dict, outputs: dict) -> None:
    """The assertions about a ranking's outputs that do not depend on the order the atomics give: for the reference's outputs and
    the device's alike.  Positions inside one bucket are never compared."""
    p = inputs["params"]
    info = dict(zip(INFO_WORDS, (int(x) for x in outputs["info"])))
    tile_cost = np.asarray(inputs["tile_cost"], np.int64)
    order = np.asarray(outputs["tile_order"], np.int64)
    assert sorted(order.tolist()) == list(range(p["n_tiles"])), "tile_order is not a permutation of the tiles"
    assert np.all(np.diff(buckets_of(tile_cost)[order]) >= 0), "tile_order: a cheaper bucket before a dearer one"
    heavy_t = thresholds(inputs["total"], p["n_pixels"], (p["heavy_factor"], p["sparse_factor"], p["tier1_factor"]), p["sparse_stride"])[0]
    est = estimates(inputs["cost"], p["nx"], p["smooth_percent"])
    pixels, _, _ = listing(inputs["cost"], est, heavy_t)
    cost_in, cost_out = np.asarray(inputs["cost"], np.int64), np.asarray(outputs["cost_out"], np.int64)
    if info["heavy_items"] > 0:
        got = np.asarray(outputs["heavy_pixels"], np.int64)[:info["heavy_items"]]
        assert len(set(got.tolist())) == len(got), "heavy_pixels lists a pixel twice"
        assert set(got.tolist()) == set(pixels.tolist()), "heavy_pixels is not the set of pixels at or above the heavy threshold"
        assert np.all(np.diff(buckets_of(est[got])) >= 0), "heavy_pixels: a cheaper bucket before a dearer one"
        assert np.array_equal(np.flatnonzero(cost_out & FLAG), pixels), "the flagged pixels are not the listed ones"
        assert np.array_equal(cost_out & MASK, cost_in & MASK), "the ranking changed the low 31 bits of a cost"
        assert info["heavy_threshold"] == heavy_t
    else:
        assert info["heavy_threshold"] == NO_LIST, "no list, but a heavy threshold"
    assert info["tier1_items"] + info["tier2_items"] <= info["heavy_items"]
    per_wave2 = 64 // p["sparse_stride"] if p["sparse_stride"] > 0 else 0
    assert info["tier2_items"] <= info["sparse_wgs"] * p["waves_per_wg"] * per_wave2
    assert info["tier1_wgs"] <= p["tier_wgs_cap"]
    assert (info["tier1_items"] == 0) == (info["tier1_wgs"] == 0)
    assert info["sparse_wgs"] + info["semi_wgs"] <= p["max_grid"] * p["sparse_percent"] // 100
    assert info["main_skip_wgs"] < max(1, p["normal_need"] + info["sparse_wgs"] + info["semi_wgs"])


# ---------------------------------------------------------------------------------------------------------------- the cost prior
def local_to_global_row(lrow: int, tile_rows: int, tile_first: int, tile_stride: int) -> int:
    """Global row of local row `lrow` of a call that renders every tile_stride-th band of tile_rows rows from band tile_first."""
    t = lrow // tile_rows
    return (tile_first + t * tile_stride) * tile_rows + (lrow - t * tile_rows)


def local_rows(ny: int, tile_rows: int, tile_first: int, tile_stride: int) -> int:
    bands = (ny + tile_rows - 1) // tile_rows
    return sum(min((t + 1) * tile_rows, ny) - t * tile_rows for t in range(tile_first, bands, tile_stride))


def prior(cal, nx: int, ny: int, tile_rows: int, tile_first: int, tile_stride: int):
    """The cost prior of a call's rows: every pixel gets the maximum over the 3 x 3 calibration pixels around its place (ci, cj) in
    the calibration grid cal[cal_ny][cal_nx] (row 0 = bottom, as the frame), cj from the pixel's GLOBAL row.  Returns the
    per-pixel costs [local_rows][nx], the sums per 8 x 8 tile of the local row grid (modulo 2^32, as the device's counters) and
    the total."""
    cal = np.asarray(cal, np.int64)
    cal_ny, cal_nx = cal.shape
    rows = local_rows(ny, tile_rows, tile_first, tile_stride)
    cost = np.zeros((rows, nx), np.int64)
    for lrow in range(rows):
        j = local_to_global_row(lrow, tile_rows, tile_first, tile_stride)
        cj = min(cal_ny - 1, (j * cal_ny) // ny)
        for i in range(nx):
            ci = min(cal_nx - 1, (i * cal_nx) // nx)
            cost[lrow, i] = int(cal[max(cj - 1, 0):cj + 2, max(ci - 1, 0):ci + 2].max())
    tiles_x, tiles_y = (nx + 7) // 8, (rows + 7) // 8
    tile_cost = np.zeros((tiles_y, tiles_x), np.int64)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            tile_cost[ty, tx] = int(cost[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].sum())
    return cost.astype(np.uint32), (tile_cost % (1 << 32)).astype(np.uint32).ravel(), int(cost.sum())


def calibration_field(cal_nx: int, cal_ny: int) -> np.ndarray:
    """An asymmetric calibration grid: a smooth ramp that differs along both axes, a bright blob off-centre and a different
    value in each corner, so that a flip, a transpose or a row taken from the wrong band changes the prior."""
    y, x = np.mgrid[0:cal_ny, 0:cal_nx].astype(np.int64)
    cal = 20 + (3 * x) % 17 + (5 * y) % 23 + x // 7 + 2 * (y // 5)
    bx, by = (2 * cal_nx) // 3, cal_ny // 4
    r2 = (x - bx) ** 2 + 2 * (y - by) ** 2
    cal = cal + np.where(r2 < max(4, (cal_nx * cal_ny) // 40), 900 - np.minimum(r2, 800), 0)
    cal[0, 0], cal[0, -1], cal[-1, 0], cal[-1, -1] = 1111, 2222, 3333, 4444
    return cal.astype(np.uint32)


# ------------------------------------------------------------------------------------------------------- the inputs of the tests
SIZES = ((96, 64), (264, 256), (100, 37), (8, 8))    # nx x local rows: 96 tiles (the host's gate is 64); 1056 tiles and 67 584 pixels
                                                     # (every strided loop runs more than once); ragged; one tile (seam only)


def _factor(x10: int) -> np.float32:
    return np.float32(x10) / np.float32(10.0)       # as rank_pixels (rt_abi.hip): (float)x10 / 10.0f


def base_params(nx: int, rows: int, family: str) -> dict:
    """The parameter sets rank_pixels (rt_abi.hip) fills on an MI355X (256 CUs), by kernel family and share:
    "lean": whole frames of the lean family (2 x 512 threads per CU; tier workgroups fit beside the main grid);
    "lean_half" / "lean_quarter": its two share rows; "general": whole frames of the other families (3 x 256 threads per CU,
    a tier workgroup takes a main workgroup's slot)."""
    n_tiles = ((nx + 7) // 8) * ((rows + 7) // 8)
    lean = family != "general"
    threads = 512 if lean else 256
    p = dict(n_pixels=nx * rows, n_tiles=n_tiles, heavy_cap=262144, max_grid=256 * (2 if lean else 3), waves_per_wg=threads // 64,
             normal_need=(n_tiles * 64 + threads - 1) // threads, sparse_stride=8, semi_stride=1 if lean else 0, sparse_percent=35,
             sparse_work_percent=5, tier_possible=1, tier1_pixels=1536, tier1_depth=3, tier_wgs_cap=512 if lean else 384,
             tier_waves_per_main_wg=0 if lean else 4, nx=nx, smooth_percent=0,
             heavy_factor=_factor(20), sparse_factor=_factor(40), tier1_factor=_factor(45))
    if family == "lean_half":
        p.update(tier1_factor=_factor(40), sparse_percent=80)
    elif family == "lean_quarter":
        p.update(tier1_pixels=8192, tier1_factor=_factor(20), tier1_depth=4, heavy_factor=_factor(15), sparse_factor=_factor(20), sparse_percent=80,
                 sparse_work_percent=40)
    elif family == "general":
        p.update(tier1_factor=_factor(70), tier1_pixels=256, tier1_depth=1)
    else:
        assert family == "lean", family
    return p


def tile_sums(cost, nx: int, rows: int) -> np.ndarray:
    """Sums of the costs' low 31 bits per 8 x 8 tile of the nx x rows grid (row-major tiles), as uint32."""
    c = (np.asarray(cost, np.int64) & MASK).reshape(rows, nx)
    ty, tx = (rows + 7) // 8, (nx + 7) // 8
    pad = np.zeros((ty * 8, tx * 8), np.int64)
    pad[:rows, :nx] = c
    return (pad.reshape(ty, 8, tx, 8).sum(axis=(1, 3)) % (1 << 32)).astype(np.uint32).ravel()


def cost_field(kind: str, nx: int, rows: int, params: dict) -> np.ndarray:
    """The cost fields of the tests (uint32[n_pixels]), from a fixed generator per kind and size."""
    n = nx * rows
    rng = np.random.default_rng([n, sum(map(ord, kind))])
    if kind == "uniform":
        c = rng.integers(0, 201, n)
    elif kind == "equal":
        c = np.full(n, 57)
    elif kind == "two":
        c = np.where(rng.random(n) < 0.04, 300, 10)
    elif kind in ("tail", "stale"):
        c = rng.integers(30, 51, n)
        dear = rng.random(n) < 0.03
        c[dear] = rng.integers(380, 421, int(dear.sum()))
        c[rng.choice(n, 3, replace=False)] = 5000
        if kind == "stale":
            c = c | np.where(rng.random(n) < 0.1, FLAG, 0)
    elif kind == "huge":
        c = rng.integers(0, 41, n)
        c[int(rng.integers(0, n))] = 0x7FFFFFFF
    elif kind == "zero":
        c = np.zeros(n, np.int64)
    elif kind == "edges":
        # estimates exactly on, one below and one above each of the three thresholds (smooth_percent 0: a pixel's estimate is its
        # cost): the sum is fixed first (mean 50), the thresholds follow from it, and the other pixels are filled to that sum
        total = 50 * n
        ts = thresholds(total, n, (params["heavy_factor"], params["sparse_factor"], params["tier1_factor"]), 1)
        special = [t + d for t in ts for d in (-1, 0, 1)]
        rest, n_rest = total - sum(special), n - len(special)
        assert rest >= 0 and rest // n_rest + 1 < min(special), "the filler pixels must stay below every threshold"
        c = np.full(n, rest // n_rest)
        c[:rest % n_rest] += 1
        c[n_rest:] = special
        c = c[rng.permutation(n)]
        assert int(c.sum()) == total
    else:
        raise ValueError(kind)
    return c.astype(np.uint32)


# (size index, cost field, parameter family, overrides of the parameters, total as a multiple of the costs' sum)
_CASES = (
    (0, "tail", "lean", {}, 1),
    (0, "tail", "lean_half", {}, 1),
    (0, "tail", "lean_quarter", {}, 1),
    (0, "tail", "general", {}, 1),
    (1, "tail", "lean", {}, 1),
    (1, "tail", "lean_quarter", {}, 1),
    (1, "tail", "general", {}, 1),
    (1, "uniform", "lean_quarter", {}, 1),
    (1, "stale", "lean_half", {}, 1),
    (1, "two", "lean", {}, 1),
    (1, "edges", "lean", {}, 1),
    (1, "huge", "lean", {}, 1),
    (2, "tail", "lean", {}, 1),
    (2, "stale", "general", {}, 1),
    (2, "edges", "lean_quarter", {}, 1),
    (2, "two", "lean", {"smooth_percent": 90}, 1),
    (0, "tail", "lean_half", {"smooth_percent": 100}, 1),
    (3, "tail", "lean", {}, 1),
    (3, "edges", "general", {}, 1),
    (3, "uniform", "lean_quarter", {"smooth_percent": 100}, 1),
    (0, "equal", "lean", {}, 1),
    (0, "zero", "lean", {}, 1),
    (2, "equal", "lean_quarter", {"smooth_percent": 90}, 1),
    (0, "edges", "lean_half", {}, 1),
    (0, "huge", "general", {}, 1),
    (0, "two", "lean_quarter", {"sparse_work_percent": 100}, 1),
    (0, "tail", "lean", {}, 2),                                                 # the prior path ranks on a counter of its own
    (0, "tail", "lean", {"sparse_stride": 0}, 1),
    (0, "tail", "lean", {"sparse_stride": 2, "semi_stride": 4}, 1),
    (2, "tail", "lean_quarter", {"sparse_stride": 64, "semi_stride": 0}, 1),
    (0, "tail", "lean_quarter", {"tier_possible": 0}, 1),
    (0, "tail", "lean_quarter", {"tier1_pixels": 0}, 1),
    (1, "tail", "lean_quarter", {"tier1_depth": 1, "tier_wgs_cap": 16}, 1),     # more tier-1 workgroups than the tier grid has
    (1, "tail", "lean_quarter", {"tier1_pixels": 100, "smooth_percent": 90}, 1),
    (0, "tail", "general", {"tier_waves_per_main_wg": 0, "sparse_work_percent": 100}, 1),
    (0, "tail", "general", {"tier_waves_per_main_wg": 3, "max_grid": 6, "tier1_factor": _factor(20), "tier1_depth": 1,
                            "sparse_work_percent": 100, "sparse_percent": 50}, 1),   # the tier waves want more slots than the grid has
    (1, "tail", "lean", {"sparse_work_percent": 1}, 1),
    (1, "tail", "lean_quarter", {"sparse_work_percent": 100, "max_grid": 40, "sparse_percent": 35, "tier_possible": 0}, 1),   # sparse and semi workgroups hit the cap
    (2, "tail", "lean", {"heavy_cap": 64}, 1),                                  # more listed pixels than the list holds (VERDICT, cliff 1)
    (2, "tail", "lean", {"heavy_cap": 114}, 1),                                 # ... and exactly as many
    (2, "uniform", "lean", {"heavy_factor": _factor(10), "sparse_factor": _factor(10)}, 1),   # half the pixels qualify
    (0, "tail", "lean_quarter", {"max_grid": 4, "sparse_percent": 100, "sparse_work_percent": 100, "waves_per_wg": 1, "tier_possible": 0}, 1),   # no ordinary workgroup left
    (3, "tail", "lean_quarter", {"heavy_cap": 8, "sparse_work_percent": 100}, 1),
    # a list from 0.001x the mean: a fifth of the small pixels beside the one at 2^31 - 1, all of them in the sort's last bucket,
    # whose midpoint (half a million rays) is then what the admission counts for each
    (1, "huge", "lean", {"heavy_factor": np.float32(0.001)}, 1),
    (1, "huge", "lean_quarter", {"heavy_factor": np.float32(0.001), "sparse_work_percent": 100}, 1),
)


def rank_cases():
    """The inputs of the ranking tests: (id, {params, cost, tile_cost, total}) for every row of _CASES."""
    out = []
    for k, (size, kind, family, over, times) in enumerate(_CASES):
        nx, rows = SIZES[size]
        p = base_params(nx, rows, family)
        p.update(over)
        cost = cost_field(kind, nx, rows, p)
        total = times * int((cost.astype(np.int64) & MASK).sum())
        name = f"{k:02d}-{nx}x{rows}-{kind}-{family}" + "".join(f"-{a}={float(b):g}" for a, b in over.items()) + (f"-total*{times}" if times != 1 else "")
        out.append((name, {"params": p, "cost": cost, "tile_cost": tile_sums(cost, nx, rows), "total": total}))
    return out
