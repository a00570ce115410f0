"""Sessions on one resident DeviceScene (tests/session_expect.py; DESIGN.md, "What a scene carries between calls"): seeded
sequences of 30-45 calls -- camera, sphere, instance and option changes, plain, ranked, pending, progressive, adaptive and
variance frames of five frame geometries, feature buffers and ray queries -- in which every ordered pair of kinds is adjacent
at least once per scene.  After every call everything it wrote is compared, bit for bit, with the CPU oracle of the description
D' the scene should now equal (rt_render frames, their ray counts, rt_trace_rays) or with the same call on a scene freshly
created from D' under the shipped options (every other entry).  A failure names the step, the op, the last mutator and prints
the prefix for session_expect.replay().

The generator, the model and the runner are tested without a device in tests/test_scene_sessions_host.py.  A cut-down
sequence that once failed goes into REGRESSIONS below."""
import pytest

import session_expect as se

pytestmark = pytest.mark.gpu

CASES = [(name, k) for name, cfg in se.SCENES.items() for k in range(cfg["sequences"])]
# id -> (scene, ops): sequences cut down by hand from a failure, kept as cases of their own beside the generated ones
REGRESSIONS = {}


@pytest.mark.parametrize("name,k", CASES, ids=[f"{name}-{k}" for name, k in CASES])
def test_session_matches_fresh_scenes(gpu, orc, name, k):
    sequences = se.generate(name)
    assert len(sequences) == se.SCENES[name]["sequences"]
    log = se.run(se.Session(name, se.GpuBackend(gpu, orc), f"{name}-{k}"), sequences[k])
    assert len(log) == len(sequences[k]) and all(log)


if REGRESSIONS:
    @pytest.mark.parametrize("case", list(REGRESSIONS))
    def test_regression_sequence(gpu, orc, case):
        name, ops = REGRESSIONS[case]
        se.replay(name, ops, se.GpuBackend(gpu, orc))


def test_replay_of_a_prefix_is_the_same_session(gpu, orc):
    """The first half of a sequence on a new scene compares the same things and sees the same bits as the full run did at those
    steps: what a failure report prints can be trusted to show the failure again."""
    name = "general"
    ops = se.generate(name)[0]
    full = se.run(se.Session(name, se.GpuBackend(gpu, orc), f"{name}-0"), ops)
    half = ops[:len(ops) // 2]
    while half[-1]["kind"] == "render_ranked" and half[-1]["mode"] == "pending":      # (its finish() would come from another call)
        half = half[:-1]
    assert len(half) >= 10
    again = se.replay(name, half, se.GpuBackend(gpu, orc))
    assert len(again) == len(half)
    for i, (a, b) in enumerate(zip(again, full)):
        assert a == b, f"step {i}, op {ops[i]!r}: the replay compared {a}, the full run {b}"
