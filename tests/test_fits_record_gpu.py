"""The per-group fit entries, held to a recording: every case of tests/fits_record.py must launch the kernel string and return, byte for
byte, the arrays recorded for it (tests/fits_record.json) before the entries were rewritten on the scratch carver -- a change of host code
alone leaves the launches, their order and every offset in the work buffers as they were, so every output stays bit-identical.  Refused
calls are held to their exception type, error code and message.  An output the recorded commit itself did not reproduce between its two
runs is listed under "unstable" in the file and left out (scripts/record_fits.py: at most 3 such (case, dtype, field) triples, never
every field of a case)."""
import pytest

import fits_record as FR

COMMIT, RECORDED = FR.load()
PARAMS = [(c, dt) for c in FR.CASES for dt in ("f64", "f32")]


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
    assert FR.frame_digest(case, FR.DTYPES[dt]) == rec["input"], FR.DRIFTED
    got = FR.run(eng, case, FR.DTYPES[dt])
    if "rejected" in rec:
        assert got == ("rejected", *rec["rejected"]), got
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


def test_the_field_tables_are_the_front_end_s():
    from polars_ols_amd import _lib as L

    assert FR.OWN == {"ridge_cv": L.RIDGE_CV_FIELDS, "rlm": L.RLM_FIELDS, "elastic_net_cv": L.ENET_CV_FIELDS, "glm": L.GLM_FIELDS,
                      "iv2sls": L.IV_FIELDS, "absorb": L.ABSORB_FIELDS, "absorb2": L.ABSORB2_FIELDS, "glsar": L.GLSAR_FIELDS}


def test_the_recorded_commit_reproduced_itself():
    unstable = [(cid, dt, f) for (cid, dt), e in RECORDED.items() for f in e.get("unstable", {})]
    assert len(unstable) <= 3, unstable
    for e in RECORDED.values():
        assert "rejected" in e or e["outputs"], "every field of a case was unstable"


def test_frames_are_what_was_recorded():
    for c, dt in PARAMS:
        assert FR.frame_digest(c, FR.DTYPES[dt]) == RECORDED[(c["id"], dt)]["input"], FR.DRIFTED
