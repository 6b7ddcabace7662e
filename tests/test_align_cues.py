"""CPU tests of the cue-anchored forced alignment (align_long.force_align_cues): the SRT / WebVTT parser, the cue frames, the window
planning and the cue -> row-window mapping with their validity (tests/dtw_windows_ref.py's check), the refusals, and the rounds and the
result against a scripted aligner built from a planted truth -- a "recording" whose unit boundaries are known encoder frames."""
import importlib
import math

import numpy as np
import pytest

import dtw_windows_ref as wref

SOT_LEN = 3
UNIT_LIMIT = 448 - SOT_LEN - 2


@pytest.fixture(scope="module")
def al():
    return importlib.import_module("whisper-char-alignment_amd.align_long")


@pytest.fixture(scope="module")
def lf():
    return importlib.import_module("whisper-char-alignment_amd.longform")


# ---------------------------------------------------------------------------------------------- parser
SRT = """1
00:00:01,000 --> 00:00:02,500
<i>Hello</i> there,
{\\an8}second line

2
00:00:03.250 --> 00:00:04.000
Both <b>separators</b> work

3
01:02:03,004 --> 01:02:04,050

4
00:00:05,000 --> 00:00:06,000
last  one
"""

VTT = "\ufeff" + """WEBVTT - a title

NOTE this is a comment
that spans lines

STYLE
::cue { color: red }

intro
00:01.000 --> 00:02.500 align:start position:10%
<v Speaker>Hello</v> <c.yellow>there</c>,
second <00:01.500>line

NOTE another

00:00:03.250 --> 00:00:04,000
no identifier here
"""


def test_parse_srt(lf):
    assert lf.parse_cues(SRT) == [(1.0, 2.5, "Hello there, second line"), (3.25, 4.0, "Both separators work"), (3723.004, 3724.05, ""),
                                  (5.0, 6.0, "last one")]
    assert lf.parse_cues(SRT.replace("\n", "\r\n")) == lf.parse_cues(SRT)


def test_parse_vtt(lf, tmp_path):
    want = [(1.0, 2.5, "Hello there, second line"), (3.25, 4.0, "no identifier here")]
    assert lf.parse_cues(VTT) == want
    p = tmp_path / "a.vtt"
    p.write_text(VTT, encoding="utf-8")
    assert lf.read_cues(str(p)) == want
    assert lf.parse_cues("") == [] and lf.parse_cues("WEBVTT\n") == []


def test_cue_frames_floor_and_ceil(al):
    assert al.cue_frames(1.2, 1.2) == (60, 60)        # 1.2 * 50 is 60 up to rounding: neither 59 nor 61
    assert al.cue_frames(1.201, 1.201) == (60, 61)
    assert al.cue_frames(0.0, 0.019) == (0, 1)
    assert al.cue_frames(3.25, 4.0) == (162, 200)


# ---------------------------------------------------------------------------------------------- planted truth
class Truth:
    """n_cues cues of 1..6 words of 2..7 units; unit u starts at encoder frame T[u]; cue k is spoken over [T[first unit], T[next cue's first
    unit]) minus a pause, and its times are off by up to `jitter` frames either way."""

    def __init__(self, seconds, n_cues, seed=0, jitter=20, empty_every=0):
        rng = np.random.default_rng(seed)
        self.seconds = seconds
        self.n_frames = int(seconds * 100) + 3000
        self.cue_units, self.cues, self.first_unit = [], [], []
        n_words = rng.integers(1, 7, size=n_cues)
        lens = [rng.integers(2, 8, size=n) for n in n_words]
        total = int(sum(l.sum() for l in lens))
        cuts = np.sort(rng.choice(np.arange(11, int(seconds * 50) - 10), size=total, replace=False))
        self.T = [10] + [int(c) for c in cuts]   # total + 1 strictly increasing frames: the last is where the text ends
        u = 0
        for k in range(n_cues):
            starts = [int(v) for v in np.pad(np.cumsum(lens[k]), (1, 0))]
            n = starts[-1]
            a, b = self.T[u], self.T[u + n]
            a, b = max(0, a + int(rng.integers(-jitter, jitter + 1))), b + int(rng.integers(-jitter, jitter + 1))
            b = max(a, b)
            if self.cues:
                a = max(a, int(round(self.cues[-1][0] * 50)))   # sorted by start
                b = max(a, b)
            self.first_unit.append(u)
            self.cue_units.append((list(range(1000 + u, 1000 + u + n)), starts, ["c%dw%d" % (k, j) for j in range(len(lens[k]))]))
            self.cues.append((a / 50.0, b / 50.0, "cue %d" % k))
            u += n
            if empty_every and k % empty_every == 1:   # a cue without units (music, a sound description) after it
                self.first_unit.append(u)
                self.cue_units.append(([], [0], []))
                self.cues.append((a / 50.0, b / 50.0, ""))

    def plan(self, al, **kw):
        return al.CuePlan(self.cues, self.cue_units, SOT_LEN, **kw).set_audio(self.n_frames)

    def align(self, plan, w, scores=False):
        """The scripted aligner of window w: the true frames of its units, then of the text's next unit (the eot row), window-relative and
        held inside the row windows -- which must admit the truth when the cue times are off by less than the slack."""
        seek, size, units, lo, hi = plan.request(w)
        M, off = size // 2, seek // 2
        rel = np.array([self.T[u - 1000] - off for u in units] + [self.T[units[-1] - 1000 + 1] - off])
        jump = np.clip(rel, lo, hi).astype(np.int32)
        assert len(lo) == len(hi) == len(units) + 1 and wref.invalid_reason(lo, hi, len(lo), M) is None
        self.inside = getattr(self, "inside", True) and bool((jump[:-1] == rel[:-1]).all())
        if not scores:
            return (jump,)
        return jump, (np.linspace(0.2, 0.8, len(jump)).astype(np.float32), np.ones(len(jump), np.int32))


def run(al, truth, max_batch=4, **kw):
    plan = truth.plan(al, **kw)
    calls = []

    def align_rows(requests):
        calls.append(list(requests))
        return [truth.align(plan, w, scores=plan.word_scores) for _i, w in requests]

    rounds = al.cue_rounds([plan], max_batch, align_rows)
    return plan, plan.result(), rounds, calls


# ---------------------------------------------------------------------------------------------- planning
def check_plan(al, plan, g):
    live = [k for k, c in enumerate(plan.cues) if plan.units[k]]
    seen = []
    for w, win in enumerate(plan.windows):
        members, E = plan.members[w]
        seen.extend(members)
        a = members[0]
        assert win["c0"] == a and win["c1"] == members[-1] + 1 and all(plan.cues[k]["window"] == w for k in members)
        assert win["seek"] == 2 * max(0, plan.frames[a][0] - g)
        assert E == max(plan.frames[k][1] for k in members) and 2 * (E + g) - win["seek"] <= 3000
        n_units = sum(len(plan.units[k]) for k in members)
        assert SOT_LEN + 1 + n_units + 1 <= 448
        nxt = live.index(members[-1]) + 1
        if nxt < len(live):   # the longest run: one more cue breaks one of the two limits
            k = live[nxt]
            assert 2 * (max(E, plan.frames[k][1]) + g) - win["seek"] > 3000 or n_units + len(plan.units[k]) > UNIT_LIMIT
        if w in plan.pending:
            M = win["size"] // 2
            seek, size, units, lo, hi = plan.request(w)
            assert (seek, size) == (win["seek"], win["size"]) and len(units) == n_units and len(lo) == len(hi) == n_units + 1
            assert wref.invalid_reason(lo, hi, n_units + 1, M) is None
            # the mapping, restated: cue by cue
            off, r, top = seek // 2, 0, 0
            clamp = lambda v: min(max(v, 0), M - 1)   # noqa: E731
            for n, k in enumerate(members):
                s, e = plan.frames[k]
                want_lo = 0 if n == 0 else clamp(s - g - off)
                top = M - 1 if n == len(members) - 1 else max(top, clamp(max(e, plan.frames[members[n + 1]][0]) + g - off))
                for _u in plan.units[k]:
                    assert (lo[r], hi[r]) == (want_lo, top), (w, k, r)
                    r += 1
            assert (lo[r], hi[r]) == (clamp(plan.frames[members[-1]][1] - g - off), M - 1)
    assert seen == live   # every cue with units in exactly one window, in order
    assert all(plan.cues[k]["window"] is None for k in range(len(plan.cues)) if k not in live)


@pytest.mark.parametrize("seed,slack", [(0, 1.0), (1, 0.5), (2, 2.0), (3, 0.0), (4, 1.0)])
def test_planning_and_row_windows_are_valid(al, seed, slack):
    truth = Truth(600, 220, seed=seed, jitter=int(slack * 50), empty_every=5 if seed % 2 else 0)
    plan = truth.plan(al, cue_slack=slack)
    g = math.ceil(slack * 50)
    assert plan.g == g and len(plan.windows) > 5 and plan.pending == list(range(len(plan.windows)))
    check_plan(al, plan, g)
    content = truth.n_frames - 3000
    for win, (_m, E) in zip(plan.windows, plan.members):
        assert win["size"] == min(3000, content - win["seek"], 2 * (E + g) - win["seek"])


def test_row_windows_are_valid_for_any_sorted_cues(al):
    """Random sorted cues with overlaps, zero lengths, nested and identical times, and audio that ends in the middle of them."""
    rng = np.random.default_rng(7)
    for trial in range(60):
        n = int(rng.integers(1, 40))
        starts = np.sort(rng.uniform(0, 120, size=n).round(2))
        cues = [(float(a), float(a + rng.choice([0.0, 0.3, 2.0, 9.0])), "x") for a in starts]
        if trial % 3 == 0:
            t0 = cues[n // 2][0]   # the second half all start together and end wherever they did, at most 20 s later
            cues[n // 2:] = [(t0, min(max(c[1], t0), t0 + 20.0), "x") for c in cues[n // 2:]]
        units = []
        for _c in cues:
            k = int(rng.integers(0, 30))
            units.append((list(range(k)), [0, k] if k else [0], ["w"] if k else []))
        slack = float(rng.choice([0.0, 0.1, 1.0, 3.0]))
        plan = al.CuePlan(cues, units, SOT_LEN, cue_slack=slack).set_audio(int(rng.integers(1, 14000)) + 3000)
        for w in plan.pending:
            seek, size, u, lo, hi = plan.request(w)
            assert size // 2 >= 1 and wref.invalid_reason(lo, hi, len(u) + 1, size // 2) is None, (trial, w)
        for w in set(range(len(plan.windows))) - set(plan.pending):
            assert plan.windows[w]["size"] // 2 < 1


def test_refusals_come_from_the_constructor(al):
    unit = ([1, 2], [0, 2], ["w"])
    with pytest.raises(ValueError, match="sorted"):
        al.CuePlan([(2.0, 3.0, "a"), (1.0, 4.0, "b")], [unit, unit], SOT_LEN)
    with pytest.raises(ValueError, match="before it starts"):
        al.CuePlan([(2.0, 1.0, "a")], [unit], SOT_LEN)
    with pytest.raises(ValueError, match=r"cue 1 \('too long'"):   # 28.1 s + 2 x 1 s of slack > 30 s
        al.CuePlan([(0.0, 1.0, "a"), (5.0, 33.1, "too long")], [unit, unit], SOT_LEN)
    al.CuePlan([(0.0, 1.0, "a"), (5.0, 33.0, "fits")], [unit, unit], SOT_LEN)
    al.CuePlan([(0.0, 29.0, "first cue: the slack before 0 does not count")], [unit], SOT_LEN)
    many = (list(range(UNIT_LIMIT + 1)), [0, UNIT_LIMIT + 1], ["w"])
    with pytest.raises(ValueError, match=r"cue 0 \('big'.*units"):
        al.CuePlan([(0.0, 1.0, "big")], [many], SOT_LEN)
    al.CuePlan([(0.0, 1.0, "big")], [(list(range(UNIT_LIMIT)), [0, UNIT_LIMIT], ["w"])], SOT_LEN)
    with pytest.raises(ValueError, match="negative"):
        al.CuePlan([(0.0, 1.0, "a")], [unit], SOT_LEN, cue_slack=-0.5)
    al.CuePlan([(0.0, 99.0, "no units: never planned")], [([], [0], [])], SOT_LEN)   # a cue without units is skipped, whatever its times
    with pytest.raises(ValueError, match="trim_silence"):
        al.force_align_cues_batch(None, [], [], language="en", vocab_path="x", trim_silence=3)
    with pytest.raises(ValueError, match="vocab_path"):
        al.force_align_cues_batch(None, [None], [[]], language="en", vocab_path=None)
    with pytest.raises(ValueError, match="recordings"):
        al.force_align_cues_batch(None, [None], [], language="en", vocab_path="x")


# ---------------------------------------------------------------------------------------------- rounds and result
def test_result_schema_times_and_rounds(al):
    truth = Truth(300, 110, seed=11, jitter=40, empty_every=4)
    for max_batch in (1, 4, 16):
        truth.inside = True
        plan, out, rounds, calls = run(al, truth, max_batch=max_batch, cue_slack=1.0)
        W = len(plan.windows)
        assert W >= 5 and rounds == len(calls) == math.ceil(W / max_batch) and [w for c in calls for _i, w in c] == list(range(W))
        assert all(len(c) <= max_batch for c in calls)
        assert truth.inside   # the cue times are off by less than the slack: the row windows admit the planted truth
        assert set(out) == {"words", "cues", "windows", "unaligned_words"} and out["unaligned_words"] == 0
        assert len(out["cues"]) == len(truth.cues)
        n = 0
        for k, (cue, (a, b, text)) in enumerate(zip(out["cues"], truth.cues)):
            assert set(cue) == {"start", "end", "text", "w0", "w1", "window"} and (cue["start"], cue["end"], cue["text"]) == (a, b, text)
            units, starts, words = truth.cue_units[k]
            assert cue["w0"] == n and cue["w1"] == n + len(words) and (cue["window"] is None) == (not units)
            for j, word in enumerate(out["words"][cue["w0"]:cue["w1"]]):
                assert set(word) == {"word", "start", "end", "cue"} and word["word"] == words[j] and word["cue"] == k
                u = truth.first_unit[k] + starts[j]
                assert abs(word["start"] - truth.T[u] * 0.02) < 1e-9 and abs(word["end"] - truth.T[u + starts[j + 1] - starts[j]] * 0.02) < 1e-9
                assert a - 1.0 - 1e-9 <= word["start"] <= word["end"]   # inside the cue's slack window (the end may reach the next cue)
            n = cue["w1"]
        assert n == len(out["words"])
        for win in out["windows"]:
            assert set(win) == {"seek", "size", "c0", "c1"} and 0 < win["size"] <= 3000 and win["c0"] < win["c1"]


def test_word_scores_and_unaligned_words(al):
    truth = Truth(120, 50, seed=12)
    plan, out, _rounds, _calls = run(al, truth, cue_slack=1.0, word_scores=True)
    assert all(set(w) == {"word", "start", "end", "cue", "score"} and 0.2 - 1e-6 <= w["score"] <= 0.8 + 1e-6 for w in out["words"])
    assert all(set(w) == {"seek", "size", "c0", "c1", "mean_word_score"} and 0.2 <= w["mean_word_score"] <= 0.8 for w in out["windows"])
    with pytest.raises(ValueError, match="path scores"):
        plan.receive(0, truth.align(plan, 0)[0])
    # audio that ends at 40 s: the windows past it do not run and their words stay unaligned
    plan = al.CuePlan(truth.cues, truth.cue_units, SOT_LEN, word_scores=True).set_audio(4000 + 3000)
    dead = [w for w in range(len(plan.windows)) if w not in plan.pending]
    assert dead and all(plan.windows[w]["seek"] >= 4000 - 1 for w in dead)
    rounds = al.cue_rounds([plan], 2, lambda reqs: [truth.align(plan, w, scores=True) for _i, w in reqs])
    out = plan.result()
    assert rounds == math.ceil(len(plan.pending) / 2)
    lost = [w for w in out["words"] if w["start"] is None]
    assert out["unaligned_words"] == len(lost) > 0 and all(w["end"] is None and w["score"] is None for w in lost)
    assert all(out["cues"][w["cue"]]["window"] in dead for w in lost)
    assert all(out["windows"][w]["mean_word_score"] is None for w in dead)


def test_windows_of_several_recordings_share_the_rounds(al):
    truths = [Truth(100, 40, seed=20), Truth(250, 90, seed=21), Truth(30, 8, seed=22)]
    plans = [t.plan(al) for t in truths]
    calls = []

    def align_rows(requests):
        calls.append(list(requests))
        return [truths[i].align(plans[i], w) for i, w in requests]

    W = sum(len(p.windows) for p in plans)
    assert al.cue_rounds(plans, 4, align_rows) == math.ceil(W / 4) == len(calls)
    flat = [r for c in calls for r in c]
    assert flat == [(i, w) for i, p in enumerate(plans) for w in range(len(p.windows))]   # a recording's windows side by side
    for t, p in zip(truths, plans):
        alone = run(al, t)[1]
        assert p.result() == alone


# ---------------------------------------------------------------------------------------------- command line
def test_cli_options(al):
    base = ["--audio", "a.wav", "--vocab", "v", "--output_dir", "o"]
    old = al.parse_args(base + ["--text", "t.txt"])
    assert not hasattr(old, "cues") and not hasattr(old, "cue_slack") and old.text == "t.txt"
    new = al.parse_args(base + ["--cues", "s.srt", "--cue_slack", "0.5"])
    assert new.cues == "s.srt" and new.cue_slack == 0.5 and new.text is None
    assert al._recordings(new) == [("a.wav", "s.srt")] and al._recordings(old) == [("a.wav", "t.txt")]
    with pytest.raises(SystemExit):
        al.parse_args(base + ["--text", "t.txt", "--cues", "s.srt"])
    with pytest.raises(SystemExit):
        al._recordings(al.parse_args(base))
