"""CPU: nothing hides behind the bounds of tests/test_decode_group_gpu.py. On the float64 beam search's own trace of the scenes, every index fault
of the grouped decode's cache (tests/decode_group_ref.py: simulate) moves an asserted cache element by at least 10 of its bounds; the clean
reference rebuilt through histories / group_state is the slot-by-slot walk of the loop, with zero difference; the reference agrees with the fp32
oracle model on a group's rows; and the coverage conditions of the GPU test hold on the reference trace."""
import importlib

import numpy as np
import pytest
import torch

import decode_cache_ref as R
import decode_group_ref as GR

FACTOR = 10.0   # every fault must move an asserted quantity by this many GPU bounds
CPU_SCENES = ("b1g2", "b3g5", "budget")


@pytest.fixture(scope="module")
def sc():
    return GR.group_scene()


@pytest.fixture(scope="module")
def searched(sc):
    """Per scene: the forwards, the initial tokens, the float64 search's trace and sums, computed once."""
    out = {}
    for name in CPU_SCENES:
        audios, ni, budgets, G, _ = GR.SCENES[name]
        fw = GR.Forwards(sc["ref"], GR.scene_ckv(sc, name))
        initial = GR.initial_tokens(name)
        trace, sums, _ = GR.beam_search(fw, initial, G, budgets)
        out[name] = (fw, initial, trace, sums)
    return out


def test_histories_follow_sources_and_budgets():
    trace = np.array([[[0, 7], [0, 8], [2, 5], [2, 6]], [[1, 9], [1, 3], [2, -1], [3, -1]]])
    h = GR.histories([[1, 2], [4]], trace, 2)
    assert h[0] == [[1, 2], [1, 2], [4], [4]]
    assert h[1] == [[1, 2, 7], [1, 2, 8], [4, 5], [4, 6]]
    assert h[2] == [[1, 2, 8, 9], [1, 2, 8, 3], [4, 5], [4, 6]]
    assert GR.coverage(trace, 2) == (1, 1, 0)


@pytest.mark.parametrize("name", CPU_SCENES)
def test_reference_trace_meets_the_coverage_conditions_and_its_own_check(searched, name):
    audios, ni, budgets, G, _ = GR.SCENES[name]
    fw, initial, trace, sums = searched[name]
    moved, twice, twice_later = GR.coverage(trace, G)
    print("%s: %d choices with a source that is not the identity, %d with a source continued twice, %d of those past audio 0" % (name, moved, twice, twice_later))
    assert moved >= 3 and twice >= 1 and (len(audios) == 1 or twice_later >= 1)
    # the choice check of the GPU test, run on the reference's own trace: every assertion holds and the sums are the search's
    hists, along, n_decided = GR.check_choices(name, fw, initial, trace, G, R.TOL["logits"])
    assert n_decided >= 1
    assert float(np.abs(along - sums).max()) < 1e-10
    assert hists == GR.histories(initial, trace, G)
    # a tile of 64 keys is crossed in at least one audio
    assert any(n + 1 <= 64 * k < n + s for n, s in zip(ni, budgets) for k in (1, 2))


@pytest.mark.parametrize("name", CPU_SCENES)
def test_clean_walk_is_the_rebuilt_state(searched, name):
    """simulate() with no fault, slot by slot through broadcast, appends and reorders, names exactly the slots that group_state fills from the final
    histories: zero difference, and the logits rows are a choice apart from the cache rows."""
    audios, ni, budgets, G, _ = GR.SCENES[name]
    fw, initial, trace, _ = searched[name]
    T_max = max(n + s for n, s in zip(ni, budgets))
    hists = GR.histories(initial, trace, G)
    planes, logits, fed = GR.final_state(fw.ref, fw.ckv, hists, T_max, fw)
    walked, known = fw.planes(GR.simulate(initial, trace, G), T_max)
    assert fed == [ni[r // G] + budgets[r // G] - 1 for r in range(len(fed))]
    assert [int(k.sum()) for k in known] == fed and bool(known[:, 0].all())
    assert float((walked - planes).abs().max()) == 0.0
    again, _, _ = GR.group_state(fw.ref, fw.ckv, hists[-1], T_max, fw)
    assert float((again - planes).abs().max()) == 0.0
    # group_state's own logits rows follow the rows it is given: row r's parent at the last choice
    _, own, _ = GR.group_state(fw.ref, fw.ckv, hists[-1], T_max, fw)
    for r in range(len(fed)):
        src, t = trace[-1, r]
        if t >= 0:
            assert float((own[r] - logits[src]).abs().max()) < 1e-10   # (one forward, two vocabulary products of different batches)


def test_reference_is_the_fp32_oracle_model_on_a_group(sc, searched):
    """The float64 logits of the b3g5 beams before their last choice (rows of three lengths on three recordings) against oracle.whisper_ref in fp32."""
    wref = importlib.import_module("oracle.whisper_ref")
    name = "b3g5"
    audios, ni, budgets, G, _ = GR.SCENES[name]
    fw, initial, trace, _ = searched[name]
    rows = GR.histories(initial, trace, G)[-2]
    oracle = wref.WhisperRef({k: v.float() for k, v in sc["sd"].items()}, sc["D"])
    xa = oracle.encoder(sc["mel5"][list(audios)])
    got = fw.last_logits([r // G for r in range(len(rows))], rows)
    err = 0.0
    for b in range(len(audios)):
        tokens = torch.tensor(rows[b * G:(b + 1) * G], dtype=torch.long)
        want = oracle.decoder(tokens, xa[b:b + 1].expand(G, -1, -1))[0][:, -1].double()
        err = max(err, float((got[b * G:(b + 1) * G] - want).abs().max()))
    print("float64 group reference vs fp32 oracle: max |d logits| %.2e" % err)
    assert err < 1e-4


def _fault_rows(fw, initial, trace, G, T_max, L):
    """(fault, choice, layer-0 shift, deeper shift, slots moved) for every fault that applies to the scene; the faults of one reorder at every
    choice whose reorder moves a row."""
    clean = GR.simulate(initial, trace, G)
    B = len(initial)
    live_all = [c for c in range(1, len(trace)) if (trace[c, :, 1] >= 0).all()]
    moving = [c for c in range(1, len(trace)) if any(trace[c, r, 0] != r for r in range(trace.shape[1]) if trace[c, r, 1] >= 0)]
    out = []

    def add(label, prov, c=None, planes_from_fault=None):
        out.append((label, c) + GR.plane_shift(fw, clean, prov, T_max, planes_from_fault))

    for c in moving:
        skipped = GR.simulate(initial, trace, G, "a no reorder", c)
        add("a no reorder", skipped, c)
        add("c newest slot not copied", GR.simulate(initial, trace, G, "c newest slot not copied", c), c)
        add("d last plane not reordered", skipped, c, [(L - 1, 1)])
        add("d V planes not reordered", skipped, c, [(l, 1) for l in range(L)])
        add("e source half two choices old", GR.simulate(initial, trace, G, "e source half two choices old", c), c)
    if B > 1:
        for fault in ("b source relative to the group", "f broadcast by r % B", "g cross-K/V of audio r % B", "g cross-K/V of audio r // G + 1",
                      "g cross-K/V of audio r // G - 1"):
            add(fault, GR.simulate(initial, trace, G, fault))
    if len(live_all) < len(trace) - 1:
        c = live_all[-1] + 1   # the first choice with an audio past its budget
        add("h past its budget, reordered from a neighbour", GR.simulate(initial, trace, G, "h past its budget, reordered from a neighbour", c), c)
    return out


ALL_FAULTS = {"a no reorder", "b source relative to the group", "c newest slot not copied", "d last plane not reordered", "d V planes not reordered",
              "e source half two choices old", "f broadcast by r % B", "g cross-K/V of audio r % B", "g cross-K/V of audio r // G + 1",
              "g cross-K/V of audio r // G - 1", "h past its budget, reordered from a neighbour"}


def test_every_fault_moves_an_asserted_quantity(sc, searched):
    """The fault table, in bounds moved (the larger of layer-0 shift / TOL plane0 and deeper shift / TOL plane_deep). A fault of ONE reorder (a, c,
    d, e) is listed at every choice whose reorder moves a row. It stays in the final cache when the line of a row it touched survives to the last
    choice; where every such line dies out, or the wrong row held the same values (e at a choice whose sources repeat the previous choice's; c where
    the destination and the source fed the same token), it
    moves NO asserted slot (0 slots, listed) and shows only in the logits and choices of the step behind it. What is asserted: a fault that moves
    any asserted slot moves one by at least FACTOR bounds -- nothing lands between 0 and 10 bounds --; a skipped reorder (a) at the last moving
    choice always shows; every fault reaches FACTOR bounds in the three-audio scene (h: in the budget scene, the only one with an audio past its
    budget); (b), (f) and the r % B form of (g) do not exist at B = 1."""
    L = sc["D"].n_text_layer
    print("%-8s %-46s %6s %10s %10s %7s %8s" % ("scene", "fault", "choice", "plane0", "plane_deep", "slots", "bounds"))
    failed, best = [], {}
    for name in CPU_SCENES:
        audios, ni, budgets, G, _ = GR.SCENES[name]
        fw, initial, trace, _ = searched[name]
        T_max = max(n + s for n, s in zip(ni, budgets))
        rows = _fault_rows(fw, initial, trace, G, T_max, L)
        last_a = max(c for label, c, *_ in rows if label == "a no reorder")
        for label, c, s0, sd, moved in rows:
            ratio = max(s0 / R.TOL["plane0"], sd / R.TOL["plane_deep"])
            print("%-8s %-46s %6s %10.3e %10.3e %7d %8.1f" % (name, label, "-" if c is None else c, s0, sd, moved, ratio))
            best[(name, label)] = max(best.get((name, label), 0.0), ratio)
            if (moved > 0 or (label == "a no reorder" and c == last_a)) and ratio < FACTOR:
                failed.append((name, label, c, ratio))
    assert not failed, failed
    for label in sorted(ALL_FAULTS):
        scene = "budget" if label.startswith("h ") else "b3g5"
        print("%-46s %-8s %8.1f bounds" % (label, scene, best[(scene, label)]))
        assert best[(scene, label)] >= FACTOR, (label, scene, best[(scene, label)])
    for name in CPU_SCENES:   # and the faults of one reorder in every scene
        for label in ("a no reorder", "c newest slot not copied", "d last plane not reordered", "d V planes not reordered", "e source half two choices old"):
            assert best[(name, label)] >= FACTOR, (name, label, best[(name, label)])
