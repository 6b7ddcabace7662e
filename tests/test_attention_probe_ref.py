"""CPU tests of the attention probes (tests/attention_probe_ref.py) that tests/test_attention_probes_gpu.py feeds the kernels: the inputs are
exact in f16, the peaked probe's target holds all but 1e-5 of every row's mass at every swept shape, its value rows are told apart by 0.25,
and each of the index errors the probes are meant for -- restated as a mutation of the float64 reference -- moves every row it touches by
at least 8 GPU tolerances (uniform probe) or 0.25 (peaked probe, against a GPU bound of 4e-3). So the GPU comparison hides none of them.

Which probe is meant to catch which mutation:
    drop_last_key, admit_one_more            counting errors: the uniform probe (the peaked one sees a dropped target key, not a dropped other key)
    shift_v_by_one, next_head                identity errors: the peaked probe, under every target map
    swap_adjacent_queries                    identity error: the peaked probe under `spread` (under `last` with the causal mask, where `last` gives every
                                             row its own key and `spread` gives rows 0 and 1 the same one)"""
import pytest
import torch

import attention_probe_ref as ref

PAIR_TOL = 3e-6          # the pair kernels' bound in the GPU test; the f16 kernels' is one f16 spacing of the result
CATCHES = {"drop_last_key": "uniform", "admit_one_more": "uniform", "shift_v_by_one": "peaked", "swap_adjacent_queries": "peaked",
           "next_head": "peaked"}


def _launches():
    """Every distinct launch of the GPU test as (label, planes, nh, live): planes = (batch rows, largest key count) of the input arrays."""
    seen, out = set(), []
    for name, shapes in ref.SWEEPS.items():
        for nq, nk, causal in shapes:
            if (nq, nk, causal) not in seen:
                seen.add((nq, nk, causal))
                out.append((f"{name} nq={nq} nk={nk} causal={causal}", (ref.B, ref.NK_MAX), ref.H, ref.live_counts(nq, nk, causal)))
    for shuffled in (False, True):
        live = ref.live_counts(1, ref.ROWS_B, False, counts=ref.rows_counts(shuffled), nb=ref.ROWS_B)
        out.append((f"rows shuffled={shuffled}", (ref.ROWS_B, ref.ROWS_B), ref.H, live))
    return out


LAUNCHES = _launches()


def _peaked(planes, live, name):
    k, v = ref.peaked_k(*planes, ref.H), ref.peaked_v(*planes, ref.H)
    t = ref.targets(name, live)
    return ref.peaked_q(k, t), k, v, t


def test_sweeps_hold_the_shapes_where_the_index_arithmetic_changes():
    s = ref.SWEEPS
    assert [nk for _, nk, _ in s["key"]] == list(range(1, 201)) + [255, 256, 257, 448, 1499, 1500] and {nq for nq, _, _ in s["key"]} == {97}
    assert [nq for nq, _, _ in s["query"]] == list(range(2, 261)) and {nk for _, nk, _ in s["query"]} == {70}
    assert [n for n, _, _ in s["causal"]] == list(range(1, 261)) + [448] and all(nq == nk and c for nq, nk, c in s["causal"])
    assert (37, 37, True) in s["causal"]        # the prefill form: every launch reads its keys from planes longer than nk
    assert len(s["capture"]) == 2 * 82 and {nq for nq, _, _ in s["capture"]} == {5, 69} and (69, 1500, False) in s["capture"]
    assert [n for n, _, _ in s["causal_capture"]] == [1, 5, 63, 64, 65, 130]
    assert [nk for _, nk, _ in s["decode"]] == list(range(1, 301)) and {nq for nq, _, _ in s["decode"]} == {1}
    assert [(ref.cap_cols(n), ref.cap_ld(n)) for n in (1, 4, 5, 80, 145, 1500)] == [(1, 8), (4, 8), (5, 12), (80, 84), (145, 152), (145, 152)]
    assert sorted(ref.rows_counts(True).tolist()) == ref.rows_counts(False).tolist() == list(range(1, 301))
    assert ref.rows_counts(True).tolist() != ref.rows_counts(False).tolist()
    assert max(max(nq for nq, _, _ in v) for v in s.values()) <= ref.NQ_MAX and max(max(nk for _, nk, _ in v) for v in s.values()) == ref.NK_MAX


def test_every_input_is_its_own_f16_image():
    for planes in ((ref.B, ref.NK_MAX), (ref.ROWS_B, ref.ROWS_B)):
        k, v, u = ref.peaked_k(*planes, ref.H), ref.peaked_v(*planes, ref.H), ref.uniform_v(*planes, ref.H)
        for x in (k, 4 * k, v, u):
            assert torch.equal(x.half().double(), x)
        assert set(u[:, :planes[1]].unique().tolist()) == {-2.0, 2.0} and set(k[:, :planes[1]].unique().tolist()) == {-1.0, 1.0}
        assert v[:, :planes[1]].abs().max() <= 2.0
        for x, xk in ((u, k), (v, k)):      # the guard rows: K = 0, V = 64
            assert bool((x[:, planes[1]:] == ref.GUARD_V).all()) and bool((xk[:, planes[1]:] == 0).all()) and x.shape[1] == planes[1] + ref.GUARD
        for which, hi in (("q", 4 * k), ("k", k), ("v", v)):
            lo = ref.lo_halves(hi.shape, which)
            assert torch.equal(lo.half().double(), lo) and bool((lo.abs() == ref.LO).all())
            assert torch.equal((hi + lo).float().double(), hi + lo)      # the pair sum is exact in f32: the reference takes hi + lo
    assert bool((ref.lo_halves((4, 64), "q") != ref.lo_halves((4, 64), "k")).any())


def test_spacing_f16_is_the_f16_grid():
    x = torch.tensor([0.0, 2.0 ** -20, 6.0e-5, 2.0 ** -14, 0.001, 0.75, 1.0, 1.999, 2.0, 64.0])
    h = x.half()
    nxt = torch.nextafter(h, torch.tensor(float("inf"), dtype=torch.float16))
    want = (nxt.double() - h.double())
    want[0] = 2.0 ** -24
    assert torch.equal(ref.spacing_f16(h), want)
    assert torch.equal(ref.spacing_f16(-h), want)


def test_peaked_probe_target_holds_the_mass_and_logits_are_integers():
    """At every swept shape, row and map: the logits are integers, the target's is 32, and p_target >= 1 - 1e-5 (a condition of the GPU bounds, with
    a margin of 4 over the worst row; another seed, not another bound, if it fails)."""
    worst = {}
    for label, planes, nh, live in LAUNCHES:
        for name in ref.MAPS:
            q, k, v, t = _peaked(planes, live, name)
            assert bool((t >= 0).all()) and bool((t < live).all()), (label, name)
            out, logits, p = ref.peaked_ref(q, k, v, nh, live)
            assert torch.equal(logits, logits.round()), (label, name)
            idx = t.view(t.shape[0], 1, t.shape[1], 1).expand(-1, nh, -1, 1)
            assert bool((torch.gather(logits, 3, idx) == 32).all()), (label, name)
            leak = (1 - torch.gather(p, 3, idx)).max().item()
            assert leak <= 1e-5, (label, name, leak)
            nk = int(live.max())
            worst[nk] = max(worst.get(nk, 0.0), leak)
            want = torch.gather(v, 1, t.unsqueeze(-1).expand(-1, -1, v.shape[-1]))
            assert (out - want).abs().max().item() <= 4 * 1e-5 + 1e-12, (label, name)       # |v| <= 2 on both sides of the leak
    print("largest 1 - p_target at nk = 33 / 200 / 448 / 1500:", [f"{worst[n]:.1e}" for n in (33, 200, 448, 1500)])


def test_value_rows_of_the_peaked_probe_are_told_apart():
    """Max-abs distance of two value rows j != j' < 1021 is at least 0.25 (the row formula has period 1021 in j). The two shapes with nk >= 1499
    are exempt from THIS assertion: rows j and j + 1021 are equal there, and a launch that mistook one for the other would pass; rows next to each
    other differ by 0.25 over the whole plane, which is what shift_v_by_one needs."""
    v = ref.peaked_v()[0, :ref.NK_MAX, :ref.HEAD]
    a = v[:1021]
    best = float("inf")
    for j0 in range(0, 1021, 64):
        d = (a[j0:j0 + 64, None, :] - a[None, :, :]).abs().amax(-1)
        d[torch.arange(d.shape[0]), torch.arange(j0, j0 + d.shape[0])] = float("inf")
        best = min(best, d.min().item())
    print("smallest distance between two value rows:", best)
    assert best >= 0.25
    assert torch.equal(v[1021:], v[:ref.NK_MAX - 1021])
    assert (v[1:] - v[:-1]).abs().amax(-1).min().item() >= 0.25
    assert sum(nk >= 1021 for sw in ref.SWEEPS.values() for _, nk, _ in sw) == sum(nk >= 1499 for sw in ref.SWEEPS.values() for _, nk, _ in sw)
    # head h + 1 of the same key row is the negated row: at least 2 * 0.25 away wherever a row is not all zero
    assert v.abs().amax(-1).min().item() >= 0.125


@pytest.mark.parametrize("mutate", ref.MUTATIONS)
def test_every_mutation_moves_every_row_it_touches(mutate):
    """Per mutation and swept shape: the mutated reference against the true one, the largest difference over a row's 64 channels (per head)."""
    probe = CATCHES[mutate]
    smallest = float("inf")
    for label, planes, nh, live in LAUNCHES:
        hit = ref.affected(mutate, live)
        if not bool(hit.any()):
            continue
        nb, nq = live.shape
        hit = hit.view(nb, nq, 1).expand(nb, nq, nh)
        if probe == "uniform":
            v = ref.uniform_v(*planes, nh)
            true, mut = ref.uniform_ref(v, nh, live), ref.uniform_ref(v, nh, live, mutate=mutate)
            tol = torch.maximum(ref.spacing_f16(true), torch.tensor(PAIR_TOL, dtype=torch.float64))
            move = ((mut - true).abs() / tol).view(nb, nq, nh, ref.HEAD).amax(-1)
            assert bool((move[hit] >= 8).all()), (label, move[hit].min().item())
            smallest = min(smallest, move[hit].min().item())
        else:
            causal = bool((live[:, -1] != live[:, 0]).any()) and nq > 1
            names = ref.MAPS if mutate != "swap_adjacent_queries" else (("last",) if causal else ("spread",))
            for name in names:
                q, k, v, _ = _peaked(planes, live, name)
                true, mut = ref.peaked_ref(q, k, v, nh, live)[0], ref.peaked_ref(q, k, v, nh, live, mutate=mutate)[0]
                move = (mut - true).abs().view(nb, nq, nh, ref.HEAD).amax(-1)
                assert bool((move[hit] >= 0.25).all()), (label, name, move[hit].min().item())
                smallest = min(smallest, move[hit].min().item())
    print(mutate, "smallest move of a touched row:", smallest, "GPU tolerances" if probe == "uniform" else "")
    assert smallest < float("inf")
