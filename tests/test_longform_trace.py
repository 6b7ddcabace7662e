"""CPU characterisation of the long-form host layer (whisper-char-alignment_amd: transcribe.py, align_long.py and what they share):
tests/golden/make_longform_trace.py drives transcribe / transcribe_batch / force_align_long_batch and the two command lines against a
stub model that writes every engine call down, and tests/golden/longform_trace.json holds what it recorded on the commit before the layer
was restructured. The same cases are replayed here once, and every case's call list and result must serialise to the same string as the
fixture's: the same engine calls with the same shapes and values in the same order, the same result dicts in the same key order, the same
refusals with no engine call before them. The fixture is not regenerated when the host layer is merely rearranged."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_longform_trace", os.path.join(GOLDEN, "make_longform_trace.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


gen = _load_generator()
with open(os.path.join(GOLDEN, "longform_trace.json")) as _f:
    WANT = gen.unpack(json.load(_f))
CASES = [(section, name) for section, cases in WANT.items() for name in cases]


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    return gen.run_all(str(tmp_path_factory.mktemp("longform_trace")))


def test_the_fixture_holds_the_cases_the_generator_runs(replayed):
    assert {s: list(c) for s, c in replayed.items()} == {s: list(c) for s, c in WANT.items()}
    assert os.path.getsize(os.path.join(GOLDEN, "longform_trace.json")) < 200 * 1024
    assert len(WANT["transcribe"]) >= 48 and all("raises" in c and c["calls"] == [] for c in WANT["refusals"].values())


@pytest.mark.parametrize("section,name", CASES, ids=["%s/%s" % c for c in CASES])
def test_case_replays_to_the_recorded_calls_and_results(replayed, section, name):
    got, want = replayed[section][name], WANT[section][name]
    assert list(got) == list(want)
    for key in want:   # (key by key, so that a failure names the part that moved)
        assert gen.serialise(got[key]) == gen.serialise(want[key]), "%s/%s: %s differs" % (section, name, key)
