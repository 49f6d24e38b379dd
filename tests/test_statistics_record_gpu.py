"""Statistics mode, held to a recording: every case of tests/statistics_record.py must launch the kernel string and return, byte for byte,
the arrays recorded for it (tests/statistics_record.json) before the entries moved to csrc/api_stats.hip -- the kernels sum in a fixed order
and use integer atomics only, so a change of host code alone leaves every output bit-identical.  Rejected cases are held to their error
code and message.  An output the recorded commit itself did not reproduce between its two runs is listed under "unstable" in the file and
left out (scripts/record_statistics.py: at most 3 such (case, dtype, field) triples, never every field of a case)."""
import pytest

import statistics_record as SR

COMMIT, RECORDED = SR.load()
PARAMS = [(c, dt) for c in SR.CASES for dt in ("f64", "f32")]


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,dt", PARAMS, ids=[f"{c['id']}-{dt}" for c, dt in PARAMS])
def test_case_reproduces_the_recorded_kernel_and_bytes(eng, case, dt):
    rec = RECORDED[(case["id"], dt)]
    assert SR.frame_digest(case, SR.DTYPES[dt]) == rec["input"], SR.DRIFTED
    got = SR.run(eng, case, SR.DTYPES[dt])
    if "rejected" in rec:
        assert got == ("rejected", rec["rejected"][0], rec["rejected"][1]), got
        return
    assert got[0] == "ok", got
    assert got[1] == rec["last_kernel"], (got[1], rec["last_kernel"])
    unstable = set(rec.get("unstable", {}))
    assert set(got[2]) == set(rec["outputs"]) | unstable
    differing = sorted(f for f, d in rec["outputs"].items() if got[2][f] != d)
    assert not differing, f"{differing} differ from the bytes recorded on {COMMIT}"


def test_the_recording_covers_every_case_and_every_rejection():
    assert set(RECORDED) == {(c["id"], dt) for c, dt in PARAMS}
    for c, dt in PARAMS:
        assert ("rejected" in RECORDED[(c["id"], dt)]) == bool(c.get("reject")), (c["id"], dt)


def test_the_recorded_commit_reproduced_itself():
    unstable = [(cid, dt, f) for (cid, dt), e in RECORDED.items() for f in e.get("unstable", {})]
    assert len(unstable) <= 3, unstable
    for e in RECORDED.values():
        assert "rejected" in e or e["outputs"], "every field of a case was unstable"


def test_frames_are_what_was_recorded():
    for c, dt in PARAMS:
        assert SR.frame_digest(c, SR.DTYPES[dt]) == RECORDED[(c["id"], dt)]["input"], SR.DRIFTED
