"""The sequence of C ABI calls every public method of drake_ddp_amd/ilqr.py makes - entry point, selector, byte count, buffer
contents, order - and what the method returns, against the record of the commit before the front end was split by concern
(tests/frontend_trace.json; tests/frontend_fake.py says how it was written).  The library is a recording stand-in installed as
`_capi._lib`: CPU only, no built library."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import frontend_fake  # noqa: E402

with open(os.path.join(HERE, "frontend_trace.json")) as _f:
    RECORD = frontend_fake.unpack(json.load(_f))


def test_the_record_covers_the_script():
    assert sorted(RECORD) == sorted(s[0] for s in frontend_fake.scenarios())
    assert os.path.getsize(os.path.join(HERE, "frontend_trace.json")) < 256 * 1024


@pytest.mark.parametrize("label", sorted(RECORD))
def test_calls_and_returns_are_the_recorded_ones(label, monkeypatch):
    from drake_ddp_amd import _capi
    got = frontend_fake.run(lambda fake: monkeypatch.setattr(_capi, "_lib", fake), only=label)[label]
    want = RECORD[label]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"call {i}"
    assert len(got["calls"]) == len(want["calls"]), [c[:3] for c in got["calls"]]
    assert len(got["returns"]) == len(want["returns"])
    for i, (g, w) in enumerate(zip(json.loads(json.dumps(got["returns"])), want["returns"])):
        assert g == w, f"step {i}"


def test_the_stand_in_is_gone_afterwards():
    from drake_ddp_amd import _capi
    assert not isinstance(_capi._lib, frontend_fake.FakeLibrary)
