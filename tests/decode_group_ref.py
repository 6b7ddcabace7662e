"""Test helper: the float64 reference of what a GROUPED decode (C ABI wca_decode_group: beam search and best_of, the one loop decode_run of
csrc/engine_decode.hip) leaves behind, on the position-coded checkpoint of tests/decode_cache_ref.py. G decoder rows per audio share its cross-K/V;
the prefill's cache rows are broadcast to the groups; before every step after the first choice launch_kv_reorder copies every layer's K and V rows
from one half of dec_cache into the other, row r from row src[r] of the beam merge, slots [0, key count).

  * `histories` rebuilds every decoder row's token list after each choice from a trace [S][R][2] of (absolute source row, token; -1 = past its budget);
  * `group_state` is the expected state of a list of rows: planes [L][2][R][T_max][d] with row r filled over [0, fed_r) by the K / V of its history
    without its last token on the cross-K/V of audio r // G, and the last forward's logits per row; `final_state` puts the two views of a beam search
    together: the final cache rows follow the beams AFTER the last choice (the reorder runs behind the merge), the last forward's logits rows belong to
    the beams BEFORE it;
  * `beam_search` runs tests/beam_ref.py's BeamSearch on the reference's own logits under the filters of decode_cache_ref.text_filters();
  * `simulate` walks the loop slot by slot: every cache slot is named by what it holds, (audio, the token prefix it was computed from), and the
    faults are index edits of that walk. A slot a fault leaves unwritten (stale memory of the other half) is None and is never counted.

Scenes (SCENES): audios of GROUP_AUDIO, n_initial and budget per audio, G, and the token seed chosen on the CPU from the float64 search so that the
coverage conditions of tests/test_decode_group_gpu.py hold."""
import functools
import importlib

import numpy as np
import torch

import beam_ref
import decode_cache_ref as R

# the four recordings of decode_cache_ref.AUDIO and a fifth one for the 65-row scene
GROUP_AUDIO = R.AUDIO + ((4, 144000, 0.03),)
EOT = R.N_TEXT

# name: (audio indices, n_initial per audio, budget per audio, G, token seed)
SCENES = {
    "b1g2": ((0,), (62,), (9,), 2, 1),
    "b3g5": ((0, 1, 2), (3, 60, 126), (9, 9, 9), 5, 0),
    "budget": ((1, 3), (62, 3), (10, 5), 3, 0),
    "r65": ((0, 1, 2, 3, 4), (3, 60, 62, 126, 61), (8, 8, 8, 8, 8), 13, 1),
    "r144": ((0, 1, 2, 3, 4, 0, 1, 2, 3), (3, 60, 62, 5, 59, 61, 4, 58, 63), (8,) * 9, 16, 7),
    "best_of": ((2, 0), (62, 3), (9, 9), 3, 0),
}


# max |GPU - float64| measured on an MI355X over every run of tests/test_decode_group_gpu.py (profiles/decode_group_tests.txt), a record only: the
# asserted bounds are decode_cache_ref.TOL as they stand (5.0e-3 / 4.5e-2 / 1.13e-2)
MEASURED = {"plane0": 1.33e-3, "plane_deep": 1.16e-2, "logits": 3.97e-3}


def initial_tokens(name):
    audios, ni, _, _, seed = SCENES[name]
    return [R.token_row(n, row=1000 * seed + 10 + b).tolist() for b, n in enumerate(ni)]


@functools.lru_cache(maxsize=None)
def group_scene():
    """decode_cache_ref.scene() and, computed once and left unchanged, the log-mel and the cross-K/V of the fifth recording behind its four."""
    sc = dict(R.scene())
    syn, audio = R._pkg("synthetic"), R._pkg("audio")
    wref = importlib.import_module("oracle.whisper_ref")
    s, n, a = GROUP_AUDIO[-1]
    mel5 = wref.log_mel_spectrogram(wref.pad_or_trim(torch.from_numpy(syn.synth_audio(s, n_samples=n)) * a), audio.mel_filters(80))[None]
    ckv5 = sc["ref"].cross_kv(sc["ref"].encoder(mel5))
    sc["mel5"] = torch.cat([sc["mel"], mel5])
    sc["ckv5"] = [(torch.cat([k, k5]), torch.cat([v, v5])) for (k, v), (k5, v5) in zip(sc["ckv4"], ckv5)]
    return sc


def scene_ckv(sc, name):
    """Cross-K/V per layer of the scene's audios, in the scene's order (a recording may repeat)."""
    idx = list(SCENES[name][0])
    return [(k[idx], v[idx]) for k, v in sc["ckv5"]]


class Forwards:
    """DecodeRef.forward over (audio, token list) pairs, batched over the pairs of equal audio and length, with the K / V of every forward kept so
    that a slot named (audio, prefix) is looked up in any forward that fed that prefix."""

    def __init__(self, ref, ckv_by_audio):
        self.ref, self.ckv = ref, ckv_by_audio
        self.slot = {}     # (audio, prefix tuple) -> (forward index, slot)
        self.kv = []       # per forward: (K [L, n, d], V [L, n, d])
        self.x_last = {}   # (audio, row tuple) -> the final residual stream of the row's last position [d]

    def _run(self, a, rows):
        """rows: token lists of one length on audio a -> K, V [L, m, n, d], x [m, n, d]"""
        ckv = [(k[a:a + 1].expand(len(rows), -1, -1), v[a:a + 1].expand(len(rows), -1, -1)) for k, v in self.ckv]
        K, V, x, _ = self.ref.forward(torch.tensor(rows, dtype=torch.long), ckv)
        return K, V, x

    def last_logits(self, audios, rows):
        """Logits [len(rows), V] of the last position of every row (audios[i]: the audio of rows[i]) fed in full."""
        groups = {}
        for a, row in zip(audios, rows):
            if (a, tuple(row)) not in self.x_last:
                groups.setdefault((a, len(row)), set()).add(tuple(row))
        for (a, _), uniq in groups.items():
            uniq = sorted(uniq)
            _, _, x = self._run(a, [list(k) for k in uniq])
            for j, k in enumerate(uniq):
                self.x_last[(a, k)] = x[j, -1]
        return self.ref.logits(torch.stack([self.x_last[(a, tuple(row))] for a, row in zip(audios, rows)]))

    def resolve(self, keys):
        """Makes every (audio, prefix) of keys known: one forward per prefix that no longer known one extends."""
        pending = {}
        for a, prefix in sorted(set(keys), key=lambda k: -len(k[1])):
            if (a, prefix) in self.slot:
                continue
            pending.setdefault((a, len(prefix)), []).append(prefix)
            for t in range(len(prefix)):
                self.slot.setdefault((a, prefix[:t + 1]), (("pending", prefix), t))
        done = {}
        for (a, _), prefixes in pending.items():
            K, V, _ = self._run(a, [list(p) for p in prefixes])
            for j, p in enumerate(prefixes):
                done[(a, p)] = len(self.kv)
                self.kv.append((K[:, j], V[:, j]))
        for key, (fwd, t) in list(self.slot.items()):
            if isinstance(fwd, tuple):
                self.slot[key] = (done[(key[0], fwd[1])], t)

    def planes(self, prov, T_max):
        """prov[r]: the slots of row r, each (audio, prefix) or None -> planes [L][2][R][T_max][d] (None and unfed slots 0) and known [R][T_max] bool."""
        self.resolve([s for row in prov for s in row if s is not None])
        D = self.ref.D
        out = torch.zeros(D.n_text_layer, 2, len(prov), T_max, D.n_text_state, dtype=torch.float64)
        known = torch.zeros(len(prov), T_max, dtype=torch.bool)
        for r, row in enumerate(prov):
            by_fwd = {}
            for t, s in enumerate(row):
                if s is not None:
                    fwd, at = self.slot[s]
                    by_fwd.setdefault(fwd, ([], []))[0].append(t)
                    by_fwd[fwd][1].append(at)
            for fwd, (ts, ats) in by_fwd.items():
                out[:, 0, r, ts] = self.kv[fwd][0][:, ats]
                out[:, 1, r, ts] = self.kv[fwd][1][:, ats]
                known[r, ts] = True
        return out, known


def histories(initial, trace, G):
    """initial: one token list per audio; trace [S][R][2] of (absolute source row, token). -> S + 1 lists of R token lists: before the first choice
    and after every choice. A token of -1: the row is past its budget and keeps its history."""
    rows = [list(initial[r // G]) for r in range(len(initial) * G)]
    out = [rows]
    for step in np.asarray(trace):
        assert len(step) == len(rows)
        rows = [list(rows[r]) if int(t) < 0 else rows[int(src)] + [int(t)] for r, (src, t) in enumerate(step)]
        out.append(rows)
    return out


def group_state(ref, ckv_by_audio, rows, T_max, fw=None):
    """rows: R = B G token lists (their lengths may differ, between audios and by a choice). Row r's forward fed its history without its last token
    on the cross-K/V of audio r // G. -> (planes [L][2][R][T_max][d] with row r filled over [0, fed_r), that forward's last logits [R][V], fed [R]).
    fw: the Forwards of (ref, ckv_by_audio) where a caller keeps one, so that no forward is run twice."""
    fw = fw or Forwards(ref, ckv_by_audio)
    G = len(rows) // ckv_by_audio[0][0].shape[0]
    audios = [r // G for r in range(len(rows))]
    fed = [len(row) - 1 for row in rows]
    planes, _ = fw.planes([[(a, tuple(row[:t + 1])) for t in range(n)] for a, row, n in zip(audios, rows, fed)], T_max)
    return planes, fw.last_logits(audios, [row[:-1] for row in rows]), fed


def final_state(ref, ckv_by_audio, hists, T_max, fw=None):
    """What a beam search leaves, from histories(): the cache rows of the beams after the last choice (hists[-1]) and the logits rows of the last
    forward, whose rows were the beams before the last choice (hists[-2], fed in full). -> (planes, logits, fed)."""
    fw = fw or Forwards(ref, ckv_by_audio)
    planes, _, fed = group_state(ref, ckv_by_audio, hists[-1], T_max, fw)
    G = len(hists[-1]) // ckv_by_audio[0][0].shape[0]
    return planes, fw.last_logits([r // G for r in range(len(hists[-2]))], hists[-2]), fed


def filtered_scores(logits, sums, G, first):
    """Candidate scores [R][V] float64: log-softmax over the text tokens (text_filters()) plus the row's sum; at the first choice only beam 0 of an
    audio offers candidates."""
    filtered = logits.clone()
    for f in R.text_filters():
        f.apply(filtered, None)
    scores = filtered.log_softmax(-1).numpy() + np.asarray(sums, dtype=np.float64)[:, None]
    if first:
        scores[np.arange(len(scores)) % G != 0] = -np.inf
    return filtered, scores


def beam_search(fw, initial, G, budgets):
    """The beam search on the reference model itself: beam_ref.BeamSearch on DecodeRef logits. -> (trace [S][R][2], sums [R], margins [S]: the
    smallest non-zero score gap at each choice's selection boundaries)."""
    B, S = len(initial), max(budgets)
    audios = [r // G for r in range(B * G)]
    bs = beam_ref.BeamSearch(B, G, EOT)
    rows = [list(initial[a]) for a in audios]
    sums = np.zeros(B * G)
    trace = np.zeros((S, B * G, 2), dtype=np.int64)
    margins = []
    for c in range(S):
        frozen = {b for b in range(B) if c >= budgets[b]}
        filtered, _ = filtered_scores(fw.last_logits(audios, rows), sums, G, False)
        rows, src, sums, _, gap, _ = bs.update(rows, filtered.numpy(), sums, first=c == 0, frozen=frozen)
        trace[c, :, 0] = src
        trace[c, :, 1] = [-1 if a in frozen else row[-1] for a, row in zip(audios, rows)]
        margins.append(gap)
    return trace, sums, margins


def check_choices(tag, fw, initial, trace, G, tol_logits):
    """The choices of a trace against the reference scored along the trace's own live beams. Every kept (source, token) must score at least the
    reference's G-th best of its audio minus 4 tol_logits (c + 1): a score carries at most 2 tol_logits of log-softmax error per accumulated
    choice, and two scores are compared. Where the reference's gap between its G-th and (G + 1)-th best exceeds that bound the kept set must be
    the reference's. -> (the histories, the reference's sums along the trace [R], the number of (choice, audio) pairs decided that way)."""
    trace = np.asarray(trace)
    Rn = trace.shape[1]
    audios = [r // G for r in range(Rn)]
    rows, sums, n_decided, n_all = [list(initial[a]) for a in audios], np.zeros(Rn), 0, 0
    hists = [rows]
    for c, step in enumerate(trace):
        _, scores = filtered_scores(fw.last_logits(audios, rows), sums, G, c == 0)
        bound = 4 * tol_logits * (c + 1)
        new_sums = sums.copy()
        for b in range(Rn // G):
            r0 = b * G
            if step[r0, 1] < 0:   # past its budget: copied through
                assert (step[r0:r0 + G, 1] < 0).all() and step[r0:r0 + G, 0].tolist() == list(range(r0, r0 + G)), (tag, c, b)
                continue
            block = scores[r0:r0 + G]
            flat = block.reshape(-1)
            top = np.argpartition(-flat, G + 1)[:G + 1]
            top = top[np.argsort(-flat[top], kind="stable")]
            gth, nxt = block.flat[top[G - 1]], block.flat[top[G]]
            kept = [(int(s) - r0, int(t)) for s, t in step[r0:r0 + G]]
            assert len(set(kept)) == G, (tag, c, b, kept)
            for g, (s, t) in enumerate(kept):
                assert 0 <= s < G and 0 <= t < R.N_TEXT and np.isfinite(block[s, t]), (tag, c, b, g, s, t)
                assert block[s, t] >= gth - bound, (tag, c, b, g, s, t, block[s, t], gth, bound)
                new_sums[r0 + g] = block[s, t]
            n_all += 1
            if gth - nxt > bound:
                n_decided += 1
                assert set(kept) == {(int(i) // block.shape[1], int(i) % block.shape[1]) for i in top[:G]}, (tag, c, b, kept, gth - nxt)
        sums = new_sums
        rows = [list(rows[r]) if int(t) < 0 else rows[int(s)] + [int(t)] for r, (s, t) in enumerate(step)]
        hists.append(rows)
    print("decode-group choices %s: %d of %d (choice, audio) pairs decided by the reference margin" % (tag, n_decided, n_all))
    return hists, sums, n_decided


def coverage(trace, G):
    """(choices with a source that is not the identity, choices with a source continued by two rows, of those the ones in an audio other than 0)"""
    moved = twice = twice_later = 0
    for step in np.asarray(trace)[1:]:
        live = [r for r in range(len(step)) if step[r, 1] >= 0]
        moved += any(step[r, 0] != r for r in live)
        dup = [r for r in live if sum(1 for q in live if step[q, 0] == step[r, 0]) >= 2]
        twice += bool(dup)
        twice_later += any(r >= G for r in dup)
    return moved, twice, twice_later


# ---- the loop, slot by slot, and its faults ((d), a plane left out of the reorder, is (a) on those planes only: plane_shift's planes_from_fault)
FAULTS = ("a no reorder", "b source relative to the group", "c newest slot not copied", "e source half two choices old",
          "f broadcast by r % B", "g cross-K/V of audio r % B", "g cross-K/V of audio r // G + 1", "g cross-K/V of audio r // G - 1",
          "h past its budget, reordered from a neighbour")


def simulate(initial, trace, G, fault=None, at=None):
    """The cache half the loop leaves, prov[r][t] = (audio, token prefix) the slot was computed from, or None where the fault leaves stale memory.
    fault: None or one of FAULTS, applied at choice `at` (a, c, e, h) or throughout (b, f, g)."""
    assert fault is None or fault in FAULTS, fault
    trace = np.asarray(trace)
    B, Rn = len(initial), len(initial) * G
    rows = [list(initial[r // G]) for r in range(Rn)]

    def first_rows(r):
        a = r % B if fault == "f broadcast by r % B" else r // G
        n = len(initial[r // G])   # n_keep is the destination row's n_initial; past the source's own the prefill left pad positions
        return [(a, tuple(initial[a][:t + 1])) if t < len(initial[a]) else None for t in range(n)]

    def ckv_audio(r):
        return {"g cross-K/V of audio r % B": r % B, "g cross-K/V of audio r // G + 1": (r // G + 1) % B,
                "g cross-K/V of audio r // G - 1": (r // G - 1) % B}.get(fault, r // G)

    cur, old = [first_rows(r) for r in range(Rn)], [[] for _ in range(Rn)]
    for c, step in enumerate(trace):
        live = [int(t) >= 0 for _, t in step]
        if c >= 1:   # forward c appends the newest slot of every live row
            cur = [row + [(ckv_audio(r), tuple(rows[r]))] if live[r] else row for r, row in enumerate(cur)]
        src = [int(s) for s, _ in step]
        rows = [rows[src[r]] + [int(step[r, 1])] if live[r] else rows[r] for r in range(Rn)]
        if c == 0:
            continue
        here = at is None or at == c
        new = []
        for r in range(Rn):
            n, s = len(cur[r]), src[r]
            if fault == "b source relative to the group":
                s = src[r] - (r // G) * G
            if fault == "h past its budget, reordered from a neighbour" and here and not live[r]:
                nb = r + G if r + G < Rn and live[r + G] else r - G
                s = src[nb]
            got = (cur[s] + [None] * n)[:n]
            if here and fault == "a no reorder":
                got = cur[r]
            if here and fault == "c newest slot not copied" and live[r]:
                got = got[:n - 1] + [cur[r][n - 1]]
            if here and fault == "e source half two choices old":
                got = (old[s] + [None] * n)[:n]
            new.append(list(got))
        old, cur = cur, new
    return cur


def plane_shift(fw, clean_prov, fault_prov, T_max, planes_from_fault=None):
    """max |faulty - clean| over the asserted slots both name, in the layer-0 planes and in the deeper ones, and the number of slots moved (by more
    than 1e-9: a planted position reads ONE slot, so two rows that fed the same token at a position and at its chain of targets hold the same
    values there whatever else their histories hold, up to the float64 rounding of two batches).
    planes_from_fault: the (layer, k / v) planes the fault touches (default all): the others stay clean."""
    clean, k0 = fw.planes(clean_prov, T_max)
    mut, k1 = fw.planes(fault_prov, T_max)
    if planes_from_fault is not None:
        keep = clean.clone()
        for l, kv in planes_from_fault:
            keep[l, kv] = mut[l, kv]
        mut = keep
    both = (k0 & k1)[None, None, :, :, None]
    d = ((mut - clean) * both).abs()
    moved = int((d.amax(dim=(0, 1, 4)) > 1e-9).sum())
    return float(d[0].max()), float(d[1:].max()), moved
