"""The static and dynamic entries, held to a recording: every case of tests/entries_record.py must launch the kernel string and return, byte
for byte, the arrays recorded for it (tests/entries_record.json) before their work buffers were cut by the scratch carver -- a change of
host code alone leaves the launches, their order and every offset in the work buffers as they were, so every output stays bit-identical.
An output the recorded commit itself did not reproduce between its two runs is listed under "unstable" in the file and left out
(scripts/record_entries.py: at most 3 such (case, dtype, field) triples, never every field of a case)."""
import pytest

import entries_record as ER

COMMIT, RECORDED = ER.load()
PARAMS = [(c, dt) for c in ER.CASES for dt in ("f64", "f32")]


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
    assert ER.frame_digest(case, ER.DTYPES[dt]) == rec["input"], ER.DRIFTED
    got = ER.run(eng, case, ER.DTYPES[dt])
    assert got[0] == "ok", got
    assert got[1] == rec["last_kernel"], (got[1], rec["last_kernel"])
    unstable = set(rec.get("unstable", {}))
    assert set(got[2]) == set(rec["outputs"]) | unstable
    differing = sorted(f for f, d in rec["outputs"].items() if got[2][f] != d)
    assert not differing, f"{differing} differ from the bytes recorded on {COMMIT}"


def test_the_recording_covers_every_case():
    assert set(RECORDED) == {(c["id"], dt) for c, dt in PARAMS}


def test_the_recorded_commit_reproduced_itself():
    unstable = [(cid, dt, f) for (cid, dt), e in RECORDED.items() for f in e.get("unstable", {})]
    assert len(unstable) <= 3, unstable
    for e in RECORDED.values():
        assert e["outputs"], "every field of a case was unstable"


def test_frames_are_what_was_recorded():
    for c, dt in PARAMS:
        assert ER.frame_digest(c, ER.DTYPES[dt]) == RECORDED[(c["id"], dt)]["input"], ER.DRIFTED
