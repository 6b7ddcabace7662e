"""The probe rows of tests/decode_filter_probes.py against the CPU oracle (oracle/decoding_ref.py), before any kernel sees them: the
hand-written answers are what the oracle chooses, the two other routes by which tests filter a row (tests/decode_sample_ref.filtered_row
in float64, and the batch application tests/test_beam_step_gpu.py feeds tests/beam_ref) remove exactly the oracle's tokens, and the
threshold rows flip the oracle's text mask with the sign of their margin. The kernels run on the same rows in
tests/test_decode_filter_gpu.py."""
import numpy as np
import pytest
import torch

import decode_filter_probes as P
import decode_sample_ref


@pytest.mark.parametrize("V", P.VOCABS)
def test_known_answers_are_what_the_oracle_chooses(V):
    v = P.vocab(V)
    seen = set()
    for p, r in zip(P.probes(V), P.references(V)):
        if p.kind != "ladder":
            continue
        seen.add((p.hist, p.rules, p.form, p.label))
        assert r.token == p.expect, (p.hist, p.rules, p.form, p.label, r.token, p.expect)
        # the live timestamps, element for element (the mass rule only ever removes text)
        want = np.zeros(V - v.tsb, bool)
        span = P.LIVE_TS[p.hist](v) if p.rules else (v.tsb, V - 1)
        if span:
            want[span[0] - v.tsb:span[1] - v.tsb + 1] = True
        assert np.array_equal(~r.dead[v.tsb:], want), (p.hist, p.rules, p.form, p.label)
        if p.hist == "first" and p.rules:
            assert r.dead[:v.tsb].all()
    assert len(seen) == len(P.RUNS) * len(P.FORMS) * len(P.LADDERS)
    # the examples of the issue, at the offsets of this vocabulary
    known = {(h, r): f(v) for (h, r), f in P.KNOWN.items()}
    assert known[("single_close", 1)][3] == v.tsb + v.k2 and known[("single_close", 1)][1] == v.eot
    assert known[("pair_text", 1)][3] == v.tsb + v.k2 + 1 and known[("zero_pair_text", 1)][3] == v.tsb + 1


@pytest.mark.parametrize("V", P.VOCABS)
def test_plants_are_chosen_exactly_where_they_are_live(V):
    n_live = n_dead = 0
    for p, r in zip(P.probes(V), P.references(V)):
        if p.kind != "plant":
            continue
        assert (r.token == p.expect) == (not r.dead[p.expect]), (p.hist, p.rules, p.form, p.label)
        n_live += not r.dead[p.expect]
        n_dead += bool(r.dead[p.expect])
    assert n_live > 20 and n_dead > 20, (n_live, n_dead)


@pytest.mark.parametrize("V", P.VOCABS)
def test_every_route_to_a_filtered_row_removes_the_same_tokens(V):
    ps, refs = P.probes(V), P.references(V)
    for hist, rules, form, a, b in P.groups(V):
        fl = P.filters(V, ps[a].n_init, rules)
        assert all(p.tokens == ps[a].tokens for p in ps[a:b])
        batch = torch.from_numpy(np.stack([p.logits for p in ps[a:b]])).clone()   # as test_beam_step_gpu.py filters beam_ref's input
        for f in fl:
            f.apply(batch, torch.tensor([p.tokens for p in ps[a:b]], dtype=torch.long))
        for i in range(a, b):
            assert np.array_equal(~np.isfinite(batch[i - a].numpy()), refs[i].dead), (hist, rules, form, ps[i].label)
            row64 = decode_sample_ref.filtered_row(ps[i].logits, ps[i].tokens, fl)
            assert np.array_equal(~np.isfinite(row64), refs[i].dead), (hist, rules, form, ps[i].label)
            assert not refs[i].dead.all()


@pytest.mark.parametrize("V", P.VOCABS)
def test_threshold_rows_flip_the_text_mask_with_the_sign_of_the_margin(V):
    v = P.vocab(V)
    n = 0
    for p, r in zip(P.probes(V), P.references(V)):
        if p.kind != "threshold":
            continue
        text, sign = p.expect
        live = ~r.dead
        ts = p.logits[v.tsb:][live[v.tsb:]].astype(np.float64)
        margin = float(np.log(np.exp(ts).sum())) - float(p.logits[text])   # over what the oracle leaves live: float64 of the fp32 logits
        assert abs(margin) >= P.MIN_MARGIN and (margin < 0) == (sign > 0), (p.hist, p.label, margin)
        assert r.dead[:v.tsb].all() == (margin > 0), (p.hist, p.form, p.label, margin)
        assert bool(r.dead[text]) == (margin > 0)
        assert r.token == (text if sign > 0 else P.LIVE_TS[p.hist](v)[0]), (p.hist, p.label, r.token)
        n += 1
    assert n >= 2 * 2 * 2 * 5


@pytest.mark.parametrize("V", P.VOCABS)
def test_count_rows_hold_minus_log_n(V):
    for p, r in zip(P.probes(V), P.references(V)):
        if p.kind == "count":
            assert abs(r.logprob + np.log(r.n_flat)) < 1e-12, (p.hist, p.label, r.logprob, r.n_flat)
