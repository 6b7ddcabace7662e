"""CPU tests of beam search's host side: the float64 restatement of upstream's BeamSearchDecoder / MaximumLikelihoodRanker
(tests/beam_ref.py) on hand-worked cases, the option checks of DecodingOptions(beam_size / patience / length_penalty / best_of), the seed
mix of best_of, and what wca_decode_group refuses before it touches a GPU."""
import ctypes
import importlib
import math
import os
import re

import numpy as np
import pytest

import beam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOT, V = 5, 6
LN = math.log


def _logits(*rows):
    """rows of {token: probability} -> [R, V] logits = log p, -inf elsewhere (a filtered row)."""
    out = np.full((len(rows), V), -np.inf)
    for r, row in enumerate(rows):
        assert abs(sum(row.values()) - 1.0) < 1e-12
        for t, p in row.items():
            out[r, t] = LN(p)
    return out


@pytest.fixture(scope="module")
def decoding():
    return importlib.import_module("whisper-char-alignment_amd.decoding")


def test_eot_candidate_behind_the_last_saved_beam_is_not_finished():
    # beam 0 (sum -1.0): 3 at 0.5, eot at 0.3, 4 at 0.2; beam 1 (sum -1.5): 0 at 0.6, 1 at 0.3, eot at 0.1
    # scores: (b0, 3) -1.693, (b1, 0) -2.011, (b0, eot) -2.204, (b0, 4) -2.609, (b1, 1) -2.704, (b1, eot) -3.803
    bs = beam_ref.BeamSearch(1, 2, EOT)
    nxt, src, sums, done, gap, ties = bs.update([[9, 1], [9, 2]], _logits({3: .5, EOT: .3, 4: .2}, {0: .6, 1: .3, EOT: .1}), [-1.0, -1.5])
    assert nxt == [[9, 1, 3], [9, 2, 0]] and list(src) == [0, 1] and not done and bs.finished == [[]]
    np.testing.assert_allclose(sums, [-1.0 + LN(.5), -1.5 + LN(.6)], rtol=1e-12)
    # the margins: the walk reached two candidates and looked at the third; no row had a fourth live token, so no cut
    assert ties == 0 and gap == pytest.approx(min((-1.5 + LN(.6)) - (-1.0 + LN(.3)), (-1.0 + LN(.5)) - (-1.5 + LN(.6))))


def test_eot_candidate_ahead_is_finished_and_the_beams_reorder():
    # beam 0: eot at 0.5, 3 at 0.3, 4 at 0.2 -> (b0, eot) -1.693 finished, then (b1, 0) -2.011, then (b0, 3) -2.204
    bs = beam_ref.BeamSearch(1, 2, EOT)
    nxt, src, sums, done, _, _ = bs.update([[9, 1], [9, 2]], _logits({EOT: .5, 3: .3, 4: .2}, {0: .6, 1: .3, EOT: .1}), [-1.0, -1.5])
    assert nxt == [[9, 2, 0], [9, 1, 3]] and list(src) == [1, 0] and not done
    assert [s for s, _ in bs.finished[0]] == [(9, 1, EOT)] and bs.finished[0][0][1] == pytest.approx(-1.0 + LN(.5))


@pytest.mark.parametrize("patience, want", [(0.5, 1), (None, 2), (1.0, 2), (2.0, 4)])
def test_patience_sets_how_many_finished_sequences_end_the_search(patience, want):
    bs = beam_ref.BeamSearch(1, 2, EOT, patience)
    assert bs.max_candidates == want
    # every step each beam finishes one sequence (eot is its best token) and continues with its second token
    toks, sums, steps = [[9], [9]], [0.0, -0.1], 0
    done = False
    while not done:
        toks, _, sums, done, _, _ = bs.update(toks, _logits({EOT: .5, 1: .3, 2: .2}, {EOT: .6, 3: .25, 4: .15}), sums, first=(steps == 0))
        steps += 1
        assert steps < 10
    # the first step offers beam 0's candidates only (one eot); from then on two per step
    assert len(bs.finished[0]) == want and steps == {1: 1, 2: 2, 4: 3}[want]


def test_a_list_that_fills_mid_step_keeps_the_better_sequence_only():
    # both beams' best token is eot: (b0, eot) -1.2 + ln .6, (b1, eot) -1.3 + ln .6; one slot (patience 0.5)
    bs = beam_ref.BeamSearch(1, 2, EOT, 0.5)
    _, _, _, done, _, _ = bs.update([[9, 1], [9, 2]], _logits({EOT: .6, 3: .3, 4: .1}, {EOT: .6, 0: .3, 1: .1}), [-1.2, -1.3])
    assert done and [s for s, _ in bs.finished[0]] == [(9, 1, EOT)]
    # a second audio whose list is still empty keeps the search going
    bs = beam_ref.BeamSearch(2, 2, EOT, 0.5)
    lg = _logits({EOT: .6, 3: .3, 4: .1}, {EOT: .6, 0: .3, 1: .1}, {0: .6, 3: .3, 4: .1}, {1: .6, 0: .3, 2: .1})
    _, src, _, done, _, _ = bs.update([[9, 1], [9, 2], [8, 1], [8, 2]], lg, [-1.2, -1.3, -1.0, -1.1])
    assert not done and bs.n_done() == 1 and list(src[2:]) == [2, 3] and bs.finished[1] == []


def test_exact_ties_go_to_the_lower_beam_then_the_lower_token_and_are_counted():
    # two identical beams with equal sums, and two equal tokens inside a row
    bs = beam_ref.BeamSearch(1, 2, EOT)
    nxt, src, _, _, gap, ties = bs.update([[9, 1], [9, 1]], _logits({2: .4, 3: .4, 4: .2}, {2: .4, 3: .4, 4: .2}), [-1.0, -1.0])
    assert nxt == [[9, 1, 2], [9, 1, 3]] and list(src) == [0, 0] and ties >= 2
    assert gap == np.inf or gap > 0.1


def test_finalize_tops_a_short_list_up_from_the_best_live_beams():
    bs = beam_ref.BeamSearch(2, 3, EOT)
    bs.finished[0] = [((9, 1, EOT), -0.5)]
    bs.finished[1] = [((8, 1, EOT), -0.5), ((8, 2, EOT), -0.6), ((8, 3, EOT), -0.7)]
    toks = [[9, 1, 2], [9, 1, 3], [9, 2, 4], [8, 0, 0], [8, 0, 1], [8, 0, 2]]
    out = bs.finalize(toks, [-2.0, -1.0, -1.0, -0.1, -0.2, -0.3])
    assert out[0] == [((9, 1, EOT), -0.5), ((9, 1, 3, EOT), -1.0), ((9, 2, 4, EOT), -1.0)]   # equal sums: the lower beam first
    assert out[1] == bs.finished[1]   # a full list takes nothing from the live beams


def test_ranker_and_length_penalty(decoding):
    sums, lengths = [-6.0, -3.5, -3.5, 0.0], [6, 3, 3, 0]
    # sum / length: -1.0, -1.1667, -1.1667, (empty: last)
    assert beam_ref.rank(sums, lengths) == 0 == decoding.rank_sequences(sums, lengths)
    # length_penalty 1: ((5 + n) / 6) -> -6 / (11 / 6) = -3.27, -3.5 / (8 / 6) = -2.625: the first of the equal pair wins
    assert beam_ref.rank(sums, lengths, 1.0) == 1 == decoding.rank_sequences(sums, lengths, 1.0)
    assert decoding.sequence_score(-3.5, 3, 1.0) == pytest.approx(-3.5 / (8 / 6)) and decoding.sequence_score(-3.5, 3) == pytest.approx(-3.5 / 3)
    assert beam_ref.rank([0.0, -9.0], [0, 4]) == 1 == decoding.rank_sequences([0.0, -9.0], [0, 4])   # an empty sequence ranks last
    assert beam_ref.rank([0.0, 0.0], [0, 0]) == 0 == decoding.rank_sequences([0.0, 0.0], [0, 0])


def test_group_seed_is_restated_and_keeps_sample_0(decoding):
    for s in (0, 1, 12345, (1 << 64) - 1):
        assert decoding.group_seed(s, 0) == s == beam_ref.group_seed(s, 0)
        seeds = [decoding.group_seed(s, g) for g in range(16)]
        assert seeds == [beam_ref.group_seed(s, g) for g in range(16)] and len(set(seeds)) == 16 and all(0 <= v < 1 << 64 for v in seeds)
    assert decoding.group_seed(7, 3) == 7 ^ ((3 * 0x94D049BB133111EB) % (1 << 64))


def test_option_checks(decoding):
    ok = lambda o: decoding._check_supported(o, grouped=True)   # as decode() checks its rows
    D = lambda **kw: decoding.DecodingOptions(**{"language": "en", **kw})
    ok(D(beam_size=5))
    ok(D(beam_size=5, patience=2.0, length_penalty=1.0))
    ok(D(best_of=5, temperature=0.4, seed=1))
    ok(D(length_penalty=0.5))
    with pytest.raises(ValueError, match="together"):
        ok(D(beam_size=5, best_of=5))
    with pytest.raises(ValueError, match="patience"):
        ok(D(patience=1.0))
    with pytest.raises(ValueError, match="T=0"):
        ok(D(best_of=5))
    with pytest.raises(ValueError, match="temperature 0"):
        ok(D(beam_size=5, temperature=0.4, seed=1))
    with pytest.raises(NotImplementedError, match="seed"):
        ok(D(best_of=5, temperature=0.4))   # sampling without a seed stays refused, best_of with it
    with pytest.raises(ValueError, match="length_penalty"):
        ok(D(beam_size=2, length_penalty=1.5))
    for bad in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="beam_size"):
            ok(D(beam_size=bad))
    mel = np.zeros((2, 80, 3000), np.float32)
    import torch
    for kw in ({"beam_size": 5}, {"best_of": 2}, {"patience": 1.0}, {"best_of": 2, "temperature": 0.5, "seed": 0}):
        with pytest.raises(NotImplementedError):   # a check on behalf of a decode of one row per audio refuses them as it always did
            decoding._check_supported(D(**kw))
    with pytest.raises(NotImplementedError, match="beam_size"):   # audios with different numbers of decoder rows
        decoding.decode(None, torch.from_numpy(mel), [D(beam_size=2), D()])
    with pytest.raises(ValueError, match="share best_of"):
        decoding.decode(None, torch.from_numpy(mel), [D(best_of=2, temperature=0.5, seed=1), D(best_of=3, temperature=0.5, seed=1)])


def test_decode_group_refuses_null_arguments_without_a_gpu(wca):
    lib, L = wca._lib.load(), wca._lib
    dd, gd = L.DecodeDesc(), L.GroupDesc()
    for args in ((None, None, None), (None, ctypes.byref(dd), None), (None, ctypes.byref(dd), ctypes.byref(gd))):
        assert lib.wca_test_set_switch(b"no_such_switch", 1) < 0 and b"null" not in lib.wca_last_error()
        assert lib.wca_decode_group(*args) < 0 and b"null" in lib.wca_last_error(), args
    bd = L.BeamDesc()
    for fn, args in ((lib.wca_test_beam_step, (None, None)), (lib.wca_test_beam_step, (None, ctypes.byref(bd))),
                     (lib.wca_test_kv_reorder, (None, None, None, 0, 0, 0, 0, 0, None, 0, None)), (lib.wca_test_beam_trace, (None, None, None, None, 0))):
        assert lib.wca_test_set_switch(b"no_such_switch", 1) < 0 and b"null" not in lib.wca_last_error()
        assert fn(*args) < 0 and b"null" in lib.wca_last_error(), fn.__name__
    # pointers first, then the 32-bit fields, padded to the pointers' alignment; the field lists are the header's
    assert ctypes.sizeof(gd) == 5 * 8 + 3 * 4 + 4 and ctypes.sizeof(bd) == 19 * 8 + 6 * 4
    header = open(os.path.join(ROOT, "include", "wca.h")).read()
    for name, struct in (("wca_group_desc", L.GroupDesc), ("wca_test_beam_desc", L.BeamDesc)):
        body = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, header, flags=re.S).group(1)
        assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f[0] for f in struct._fields_], name
    assert lib.wca_version() >= 18


def test_the_ladder_gives_temperature_0_rows_the_beam_and_sampled_rows_best_of(monkeypatch):
    """upstream's decode_with_fallback: beam_size and patience at temperature 0, best_of above it; a row that only rides along carries neither."""
    tr = importlib.import_module("whisper-char-alignment_amd.transcribe")
    seen = []

    def fake_decode(model, mel, rows, **kw):
        seen.append((list(rows) if isinstance(rows, (list, tuple)) else [rows], kw))
        return [None] * 2

    monkeypatch.setattr(tr.decoding, "decode", fake_decode)

    class Model:
        is_multilingual, max_batch = True, 8

    call = tr._Call(Model(), "en", None, None, {"length_penalty": 1.0, "sample_len": 9}, None, None, {}, None, (0.0, 0.4), 7, 2.4,
                    group_options=dict(beam_size=3, patience=2.0, best_of=2))
    call.decode_rung("en", [None, None], [[], [5]], [0.0, 0.0], [11, 12])
    call.decode_rung("en", [None, None], [[], [5]], [None, 0.4], [21, 22], redecode=True)
    (rung0, kw0), (rung1, kw1) = seen
    assert [(o.beam_size, o.patience, o.best_of, o.temperature, o.length_penalty) for o in rung0] == [(3, 2.0, None, 0.0, 1.0)] * 2
    assert [(o.beam_size, o.patience, o.best_of, o.temperature, o.seed, o.length_penalty) for o in rung1] == \
        [(None, None, None, 0.0, None, 1.0), (None, None, 2, 0.4, 22, 1.0)]
    assert kw1["redecode"] and kw1["row_sample_len"] == [1, None] and not kw0.get("redecode")
    # without the options the rows are what they were
    plain = tr._Call(Model(), "en", None, None, {}, None, None, {}, None)
    plain.decode_rung("en", [None, None], [[], [5]])
    assert all(o == tr.decoding.DecodingOptions(language="en", prompt=p) for o, p in zip(seen[2][0], (None, [5])))


def test_transcribe_refuses_group_options_it_cannot_run():
    tr = importlib.import_module("whisper-char-alignment_amd.transcribe")
    audio = [np.zeros(16000, np.float32)]
    with pytest.raises(ValueError, match="seed"):
        tr.transcribe_batch(None, audio, language="en", best_of=2)
    with pytest.raises(ValueError, match="patience"):
        tr.transcribe_batch(None, audio, language="en", patience=2.0)
    with pytest.raises(ValueError, match="beam_size"):
        tr.transcribe_batch(None, audio, language="en", beam_size=0)
    with pytest.raises(ValueError, match="max_batch"):   # (no model: one row)
        tr.transcribe_batch(None, audio, language="en", beam_size=5)
    with pytest.raises(ValueError, match="max_batch"):
        tr.transcribe(None, audio[0], language="en", beam_size=2, best_of=5, seed=1, temperature=(0.0, 0.5))
    args = tr.parse_args(["--audio", "a.wav", "--output_dir", "o", "--beam_size", "5", "--patience", "2", "--best_of", "5", "--length_penalty", "1"])
    assert (args.beam_size, args.patience, args.best_of, args.length_penalty) == (5, 2.0, 5, 1.0)
    assert not hasattr(tr.parse_args(["--audio", "a.wav", "--output_dir", "o"]), "beam_size")
