"""Drop-in for the reference's alignment API (timing.py:13-114): same function names, arguments, return
values and error behaviour; the arithmetic runs in libwca.so on the MI355X.

  get_attentions(mel, tokens, model, tokenizer, max_frames, medfilt_width=7, qk_scale=1.0) -> (weights, logits)
  filter_attention(attns, topk=20, w_colnorm=1, w_rownorm=1, w_coverage=0) -> (selected_attns, scores_sorted)
  force_align(ws, tokens, tokenizer, aligned_unit_type, aggregation, topk, w_colnorm, w_rownorm, w_coverage)
      -> (words, start_times, end_times, matrix, scores)

`model` is a whisper-char-alignment_amd WhisperAMD engine handle, `tokenizer` a tokenizer.Tokenizer.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .audio import HOP_LENGTH, SAMPLE_RATE, TOKENS_PER_SECOND  # noqa: F401  (re-exported like the reference)
from .retokenize import split_tokens_on_spaces

_pf = C.POINTER(C.c_float)
_pi = C.POINTER(C.c_int32)


def _engine_for(device):
    """An engine on `device` for the ops that need no weights (filter_attention / force_align / dtw)."""
    from .engine import default_engine
    return default_engine(device.index if device.index is not None else 0)


def _as_cuda_f32(t):
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t))
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("the alignment engine needs an AMD GPU; there is no CPU fallback")
        t = t.cuda()
    return t.to(torch.float32).contiguous()


def get_attentions(mel, tokens, model, tokenizer, max_frames, medfilt_width=7, qk_scale=1.0):
    """Teacher-forced forward with every cross-attention head's QK logits captured, sliced to
    `max_frames`, median filtered, scaled and softmaxed (timing.py:45-67).
    mel (n_mels, 3000) f32, tokens 1-D int64 -> weights (L, H, n, F) f32 on the GPU, logits (n, V) f32."""
    max_frames = int(max_frames)
    weights, logits = model.get_attentions(mel.unsqueeze(0), tokens.unsqueeze(0), [max_frames], medfilt_width, qk_scale)
    return weights[0], logits[0]


def filter_attention(attns, topk=20, w_colnorm=1, w_rownorm=1, w_coverage=0):
    """attns (layers, heads, tokens, frames). Returns the top-k heads as a list of (1, T, F) tensors in
    ascending score order and the sorted (score, (l, h), name) tuples (timing.py:13-43)."""
    attns = _as_cuda_f32(attns)
    eng = _engine_for(attns.device)
    L, H, n, F = attns.shape
    keff = max(0, min(int(topk), L * H))
    scores = np.zeros(L * H, dtype=np.float32)
    idx = np.zeros(max(keff, 1), dtype=np.int32)
    ssc = np.zeros(max(keff, 1), dtype=np.float32)
    eng._bind_stream()
    if keff > 0:
        _lib.check(eng._lib.wca_filter_attention(eng._h, C.c_void_p(attns.data_ptr()), L, H, n, F, keff, float(w_colnorm),
                                                 float(w_rownorm), float(w_coverage), scores.ctypes.data_as(_pf),
                                                 idx.ctypes.data_as(_pi), ssc.ctypes.data_as(_pf)))
    scores_sorted = [(float(ssc[i]), (int(idx[i]) // H, int(idx[i]) % H), "sample_layer%d_head%d" % (idx[i] // H, idx[i] % H))
                     for i in range(keff)]
    selected = [attns[l, h].unsqueeze(0) for _, (l, h), _ in scores_sorted]
    return selected, scores_sorted


def _dtw_host(eng, matrix):
    """whisper.timing.dtw(-matrix) for a host matrix through the HIP kernel."""
    m = np.ascontiguousarray(matrix, dtype=np.float32)
    N, M = m.shape
    ti = np.zeros(N + M, dtype=np.int32)
    tj = np.zeros(N + M, dtype=np.int32)
    n = C.c_int32(0)
    eng._bind_stream()
    _lib.check(eng._lib.wca_dtw(eng._h, m.ctypes.data_as(_pf), N, M, ti.ctypes.data_as(_pi), tj.ctypes.data_as(_pi), C.byref(n)))
    return ti[:n.value].astype(np.int64), tj[:n.value].astype(np.int64)


def dtw(x):
    """whisper.timing.dtw drop-in: x is the ALREADY NEGATED cost matrix, as in `dtw(-matrix)`."""
    x = torch.as_tensor(x)
    dev = x.device if x.is_cuda else torch.device("cuda:0")
    return _dtw_host(_engine_for(dev), (-x).float().cpu().numpy())


def dtw_open(x):
    """The open-end form of dtw(x) (C ABI wca_dtw_open; no counterpart upstream): x is the ALREADY NEGATED cost matrix. The path starts at
    (0, 0) and ends in the last frame at the text row n* of the smallest cost per path cell, decided exactly, the lower row on ties.
    Returns (text_indices, time_indices, end_row, score); score = cost / path length at the end cell, for diagnostics only."""
    x = torch.as_tensor(x)
    dev = x.device if x.is_cuda else torch.device("cuda:0")
    eng = _engine_for(dev)
    m = np.ascontiguousarray((-x).float().cpu().numpy(), dtype=np.float32)
    N, M = m.shape
    ti = np.zeros(N + M, dtype=np.int32)
    tj = np.zeros(N + M, dtype=np.int32)
    n, end_row, score = C.c_int32(0), C.c_int32(0), C.c_float(0)
    eng._bind_stream()
    _lib.check(eng._lib.wca_dtw_open(eng._h, m.ctypes.data_as(_pf), N, M, ti.ctypes.data_as(_pi), tj.ctypes.data_as(_pi), C.byref(n),
                                     C.byref(end_row), C.byref(score)))
    return ti[:n.value].astype(np.int64), tj[:n.value].astype(np.int64), int(end_row.value), float(score.value)


def dtw_windows(x, lo, hi):
    """The windowed form of dtw(x) (C ABI wca_dtw_windows; no counterpart upstream): x is the ALREADY NEGATED cost matrix (N, M), and text
    row i may only sit at the frames lo[i] <= j <= hi[i]. The windows must satisfy 0 <= lo <= hi <= M-1, lo[0] == 0, hi[N-1] == M-1, both
    non-decreasing and lo[i+1] <= hi[i] + 1 (else the engine refuses them before anything runs); full windows give dtw(x) bit for bit.
    Returns (text_indices, time_indices)."""
    x = torch.as_tensor(x)
    dev = x.device if x.is_cuda else torch.device("cuda:0")
    eng = _engine_for(dev)
    m = np.ascontiguousarray((-x).float().cpu().numpy(), dtype=np.float32)
    N, M = m.shape
    lo, hi = np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)
    if lo.shape != (N,) or hi.shape != (N,):
        raise ValueError("lo and hi hold one entry per text row (%d), got %s and %s" % (N, lo.shape, hi.shape))
    ti = np.zeros(N + M, dtype=np.int32)
    tj = np.zeros(N + M, dtype=np.int32)
    n = C.c_int32(0)
    eng._bind_stream()
    _lib.check(eng._lib.wca_dtw_windows(eng._h, m.ctypes.data_as(_pf), N, M, lo.ctypes.data_as(_pi), hi.ctypes.data_as(_pi),
                                        ti.ctypes.data_as(_pi), tj.ctypes.data_as(_pi), C.byref(n)))
    return ti[:n.value].astype(np.int64), tj[:n.value].astype(np.int64)


def path_scores(matrix):
    """The DTW of one (N, M) matrix (NOT negated: what force_align returns as `matrix`; host or device) with the per-row score of its path,
    through wca_dtw_path_scores. Returns (text_indices, time_indices, path_mean, path_cells): the path as dtw(-matrix) gives it, and for
    every text row the float32 mean of `matrix` over the path's cells in that row and their int32 count (a column the path leaves
    vertically counts in both rows)."""
    matrix = torch.as_tensor(matrix) if not isinstance(matrix, torch.Tensor) else matrix
    if matrix.dim() != 2:
        raise ValueError("matrix must be (N, M)")
    m = _as_cuda_f32(matrix)
    jump, _end, mean, cells = _engine_for(m.device).dtw_path_scores(m.unsqueeze(0))
    # row i holds the frames jump[i] .. jump[i] + cells[i] - 1
    text_indices = np.repeat(np.arange(len(cells[0]), dtype=np.int64), cells[0])
    time_indices = np.concatenate([np.arange(j, j + c, dtype=np.int64) for j, c in zip(jump[0], cells[0])])
    return text_indices, time_indices, mean[0], cells[0]


def force_align_long(model, audio, text, **kw):
    """Word times of a recording of any length against its given transcript: align_long.force_align_long."""
    from . import align_long
    return align_long.force_align_long(model, audio, text, **kw)


def force_align_cues(model, audio, cues, **kw):
    """Word times of a recording against its subtitle cues [(start_s, end_s, text)] or an .srt / .vtt file: align_long.force_align_cues."""
    from . import align_long
    return align_long.force_align_cues(model, audio, cues, **kw)


def force_align_cues_batch(model, audios, cues, **kw):
    """force_align_cues of several recordings, their windows sharing the rounds: align_long.force_align_cues_batch."""
    from . import align_long
    return align_long.force_align_cues_batch(model, audios, cues, **kw)


def force_align_long_batch(model, audios, texts, **kw):
    """force_align_long of several recordings in lock-step: align_long.force_align_long_batch."""
    from . import align_long
    return align_long.force_align_long_batch(model, audios, texts, **kw)


def trim_words_to_speech(words, segments):
    """Pause-aware word times: the DTW gives every frame to some unit, so a word's end is the next word's start and a pause counts as
    part of the word before it. words: [{"start", "end", ...}] in seconds; segments: (start, stop) frame pairs of 10 ms in order, as
    WhisperAMD.speech_segments returns them. Word by word, with a = round(start * 100) and b = round(end * 100): if segments intersect
    [a, b) the word becomes [max(a, start of the first of them), min(b, stop of the last of them)) / 100; otherwise, and where start or
    end is None, the word is unchanged. Returns new dicts; no other key is touched."""
    out = []
    for w in words:
        w = dict(w)
        out.append(w)
        if w.get("start") is None or w.get("end") is None:
            continue
        a, b = round(w["start"] * 100), round(w["end"] * 100)
        met = [(int(x), int(y)) for x, y in segments if x < b and y > a]
        if met:
            w["start"], w["end"] = max(a, met[0][0]) / 100, min(b, met[-1][1]) / 100
    return out


def median_filter(x, filter_width):
    """whisper.timing.median_filter drop-in (reflect padding, last axis)."""
    x = _as_cuda_f32(x)
    if x.shape[-1] <= filter_width // 2:
        return x
    assert filter_width > 0 and filter_width % 2 == 1, "`filter_width` should be an odd number"
    eng = _engine_for(x.device)
    out = torch.empty_like(x)
    F = x.shape[-1]
    eng._bind_stream()
    _lib.check(eng._lib.wca_median_filter(eng._h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), x.numel() // F, F,
                                          int(filter_width)))
    return out


def force_align(ws, tokens, tokenizer, aligned_unit_type="subword", aggregation="mean", topk=-1, w_colnorm=1.0,
                w_rownorm=1.0, w_coverage=0.0):
    """ws (layers, heads, tokens, frames) attention weights -> (words, start_times, end_times, matrix, scores)
    exactly as timing.py:69-114: aggregate heads, drop the sot rows and the last row, DTW on the negated
    matrix, merge token jumps into word start/end times. Returns [[], [], [], [], None] when the text has
    at most one word (timing.py:106-107)."""
    sot_len = len(tokenizer.sot_sequence)
    scores = None
    if aggregation == "grad_norm":  # passthrough branch (timing.py:99-100): ws is already a (tokens, frames) matrix
        matrix = torch.as_tensor(ws)[sot_len:-1].float().cpu()
        dev = ws.device if isinstance(ws, torch.Tensor) and ws.is_cuda else torch.device("cuda:0")
        text_indices, time_indices = _dtw_host(_engine_for(dev), matrix.numpy())
    else:
        if aggregation == "topk":
            assert topk > 0
        elif aggregation != "mean":
            raise ValueError("aggregation must be 'mean', 'topk' or 'grad_norm'")
        ws = _as_cuda_f32(ws)
        eng = _engine_for(ws.device)
        L, H, n, F = ws.shape
        N = n - sot_len - 1
        if N < 1:
            raise ValueError("ws has %d token rows; nothing is left after the [%d:-1] slice" % (n, sot_len))
        opts = eng.make_opts(aggregation=aggregation, topk=topk, w_colnorm=w_colnorm, w_rownorm=w_rownorm,
                             w_coverage=w_coverage, sot_len=sot_len)
        mat = np.zeros((N, F), dtype=np.float32)
        ti = np.zeros(N + F, dtype=np.int32)
        tj = np.zeros(N + F, dtype=np.int32)
        plen = C.c_int32(0)
        keff = max(1, min(int(topk), L * H)) if aggregation == "topk" else 1
        sel = np.zeros(keff, dtype=np.int32)
        ssc = np.zeros(keff, dtype=np.float32)
        eng._bind_stream()
        _lib.check(eng._lib.wca_force_align(eng._h, C.c_void_p(ws.data_ptr()), L, H, n, F, C.byref(opts), mat.ctypes.data_as(_pf),
                                            ti.ctypes.data_as(_pi), tj.ctypes.data_as(_pi), C.byref(plen), sel.ctypes.data_as(_pi),
                                            ssc.ctypes.data_as(_pf)))
        matrix = torch.from_numpy(mat)
        text_indices = ti[:plen.value].astype(np.int64)
        time_indices = tj[:plen.value].astype(np.int64)
        if aggregation == "topk":
            scores = [(float(ssc[i]), (int(sel[i]) // H, int(sel[i]) % H), "sample_layer%d_head%d" % (sel[i] // H, sel[i] % H))
                      for i in range(min(int(topk), L * H))]

    words, word_tokens = split_tokens_on_spaces(list(tokens) + [tokenizer.eot], tokenizer, aligned_unit_type)
    if len(word_tokens) <= 1:
        return [[], [], [], [], None]
    word_boundaries = np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
    jumps = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    jump_times = time_indices[jumps] / TOKENS_PER_SECOND
    start_times = jump_times[word_boundaries[:-1]]
    end_times = jump_times[word_boundaries[1:]]
    return words, start_times, end_times, matrix, scores


def attention_weights(qk, max_frames, medfilt_width=7, qk_scale=1.0):
    """The post-capture half of get_attentions (timing.py:63-66) on given logits: qk (L, H, n, S) f32 (the hooked
    cross-attention logits, concatenated over layers) -> [..., :max_frames] -> median filter -> * qk_scale -> softmax."""
    qk = _as_cuda_f32(qk)
    eng = _engine_for(qk.device)
    L, H, n, S = qk.shape
    out = torch.empty(L, H, n, int(max_frames), device=qk.device, dtype=torch.float32)
    eng._bind_stream()
    _lib.check(eng._lib.wca_attention_weights(eng._h, C.c_void_p(qk.data_ptr()), L, H, n, S, int(max_frames), int(medfilt_width),
                                              float(qk_scale), C.c_void_p(out.data_ptr())))
    return out


def _default_alignment_from_weights(eng, weights, heads, text_tokens, tokenizer):
    """timing.py:159-186 on filtered + softmaxed maps `weights` (L, H, n, F): returns the reference's 5-tuple."""
    sot_len = len(tokenizer.sot_sequence)
    L, H, n, F = weights.shape
    hd = np.asarray([l * H + h for l, h in heads], dtype=np.int32)
    N = n - sot_len - 1
    norm = torch.empty(len(hd), n, F, device=weights.device, dtype=torch.float32)
    ti = np.zeros(N + F, dtype=np.int32)
    tj = np.zeros(N + F, dtype=np.int32)
    plen = C.c_int32(0)
    eng._bind_stream()
    _lib.check(eng._lib.wca_default_find_alignment(eng._h, C.c_void_p(weights.data_ptr()), L, H, n, F, hd.ctypes.data_as(_pi), len(hd),
                                                   sot_len, C.c_void_p(norm.data_ptr()), None, ti.ctypes.data_as(_pi),
                                                   tj.ctypes.data_as(_pi), C.byref(plen)))
    text_indices = ti[:plen.value].astype(np.int64)
    time_indices = tj[:plen.value].astype(np.int64)
    jumps = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    spans = default_word_spans(time_indices[jumps] / TOKENS_PER_SECOND, text_tokens, tokenizer)
    if spans is None:
        return [[], [], [], [], None]
    words, _word_tokens, _boundaries, start_times, end_times = spans
    return words, start_times, end_times, norm, None


def default_word_spans(jump_times, text_tokens, tokenizer):
    """The tail of the reference's default_find_alignment (timing.py:171-180) and of upstream's find_alignment: jump_times[i] is the time
    at which the DTW path enters text row i of text_tokens + [eot]. Returns (words, word_tokens, word_boundaries, start_times, end_times)
    -- words and word_tokens by tokenizer.split_to_word_tokens, the eot their last entry; the times one per word but that last -- or
    None when the text has at most one word. The one place this slice and boundary arithmetic is written (word_timing uses it too)."""
    words, word_tokens = tokenizer.split_to_word_tokens(list(text_tokens) + [tokenizer.eot])
    if len(word_tokens) <= 1:
        return None
    word_boundaries = np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
    jump_times = np.asarray(jump_times)
    return words, word_tokens, word_boundaries, jump_times[word_boundaries[:-1]], jump_times[word_boundaries[1:]]


def default_find_alignment(model, tokenizer, text_tokens, mel, max_frames, *, medfilt_width=7, qk_scale=1.0):
    """openai-whisper's own aligner as restated by the reference (timing.py:116-186, `--default_whisper_timing`):
    the cross-attention maps of `model.alignment_heads` (row-major (layer, head) order, like `.indices().T` of the
    reference's sparse mask) are median filtered, softmaxed, normalised per head and frame over the token axis
    ((w - mean) / std, population std), averaged, sliced [sot:-1] and aligned with DTW; words come from
    tokenizer.split_to_word_tokens. Returns (words, start_times, end_times, weights, None) where `weights` are the
    NORMALISED maps of the alignment heads, (n_heads, n, F) on the GPU, exactly the reference's 4th value."""
    tokens = torch.tensor([*tokenizer.sot_sequence, tokenizer.no_timestamps, *text_tokens, tokenizer.eot]).to(model.device)
    weights, _logits = get_attentions(mel, tokens, model, tokenizer, max_frames, medfilt_width, qk_scale)
    return _default_alignment_from_weights(model, weights.contiguous(), model.alignment_heads, text_tokens, tokenizer)


def token_logprobs(logits, tokens, tokenizer):
    """Teacher-token log-probabilities of one utterance (timing.py:146-149 in log space) through wca_token_logprobs:
    logits (n, V) f32 as get_attentions returns them, tokens the same 1-D sequence [*sot_sequence, no_timestamps, *text, eot].
    Returns a float32 GPU tensor of n_text = n - len(sot_sequence) - 2 values,
    out[i] = log_softmax(logits[len(sot_sequence) + i, :eot])[tokens[len(sot_sequence) + 1 + i]] (eot itself is not scored).
    A text token >= eot raises WcaError (upstream raises IndexError)."""
    logits = _as_cuda_f32(logits)
    sot_len = len(tokenizer.sot_sequence)
    n, V = logits.shape
    n_text = len(tokens) - sot_len - 2
    if n < len(tokens):
        raise ValueError("logits have %d rows for %d tokens" % (n, len(tokens)))
    out = torch.zeros(max(n_text, 0), device=logits.device, dtype=torch.float32)
    if n_text <= 0:
        return out
    vocab_end = int(tokenizer.eot)
    if vocab_end > V:
        raise ValueError("tokenizer.eot %d outside the logits' %d columns" % (vocab_end, V))
    rows = logits[sot_len:sot_len + n_text]
    targets = torch.as_tensor(tokens)[sot_len + 1:sot_len + 1 + n_text].to(logits.device, torch.int64).contiguous()
    eng = _engine_for(logits.device)
    eng._bind_stream()
    _lib.check(eng._lib.wca_token_logprobs(eng._h, C.c_void_p(rows.data_ptr()), n_text, V, vocab_end, C.c_void_p(targets.data_ptr()),
                                           C.c_void_p(out.data_ptr())))
    return out


def _word_boundaries(text_tokens, tokenizer, aligned_unit_type):
    """The word_boundaries of force_align / words_from_jump_frames for `text_tokens` + [eot] (char_word_starts on the char fast
    path, split_tokens_on_spaces otherwise), or None when the text has at most one word (timing.py:106-107)."""
    from .retokenize import char_word_starts
    toks = list(text_tokens) + [tokenizer.eot]
    starts = char_word_starts(toks, tokenizer) if aligned_unit_type == "char" else None
    if starts is None:
        _words, word_tokens = split_tokens_on_spaces(toks, tokenizer, aligned_unit_type)
        if len(word_tokens) <= 1:
            return None
        return np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
    return starts if len(starts) > 1 else None


def word_probabilities(token_logprobs, text_tokens, tokenizer, aligned_unit_type="char"):
    """Per-word confidence (timing.py:181-184): the mean over each word's tokens of exp(token log-prob), one value per returned word
    (aligned with force_align's / words_from_jump_frames' start_times and end_times); [] when the text has at most one word.
    token_logprobs: the n_text = len(text_tokens) values of one utterance (a row of align_batch's token log-probs, or
    token_logprobs()); a word's span is clipped to the text tokens like the reference's list slice."""
    wb = _word_boundaries(text_tokens, tokenizer, aligned_unit_type)
    if wb is None:
        return []
    lp = token_logprobs.detach().cpu().numpy() if isinstance(token_logprobs, torch.Tensor) else np.asarray(token_logprobs)
    probs = np.exp(lp[:len(text_tokens)].astype(np.float64)).tolist()
    return [float(np.mean(probs[i:j])) for i, j in zip(wb[:-1], wb[1:])]


def word_alignment_scores(path_mean, path_cells, text_tokens, tokenizer, aligned_unit_type="char"):
    """Per-word alignment score: the mean of the aggregated attention matrix over the cells of the DTW path that lie in the word's token
    rows, i.e. the cell-weighted mean sum(path_mean * path_cells) / sum(path_cells) over rows [wb[w], wb[w+1]) in float64, with the word
    boundaries of force_align / words_from_jump_frames. One value per returned word, nan for a word whose rows hold no path cell (past
    the end row of an open-end alignment); [] when the text has at most one word, like word_probabilities.
    path_mean / path_cells: one utterance's row of align_batch(path_scores=True), or path_scores()'s last two values."""
    wb = _word_boundaries(text_tokens, tokenizer, aligned_unit_type)
    if wb is None:
        return []
    to_np = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    n = len(text_tokens) + 1
    mean, cells = to_np(path_mean)[:n].astype(np.float64), to_np(path_cells)[:n].astype(np.float64)
    out = []
    for i, j in zip(wb[:-1], wb[1:]):
        c = cells[i:j].sum()
        out.append(float((mean[i:j] * cells[i:j]).sum() / c) if c > 0 else float("nan"))
    return out


def words_from_jump_frames(jump_frames, tokens, tokenizer, aligned_unit_type="char", want_words=True):
    """Host tail of the fused wca_align_batch path: `jump_frames[i]` is the frame at which the DTW path
    enters text row i (= time_indices[jumps], timing.py:110-111); returns (words, start_times, end_times)
    with the same meaning as force_align's first three outputs."""
    from .retokenize import char_word_starts
    toks = list(tokens) + [tokenizer.eot]
    starts = char_word_starts(toks, tokenizer) if aligned_unit_type == "char" else None
    if starts is None:
        words, word_tokens = split_tokens_on_spaces(toks, tokenizer, aligned_unit_type)
        if len(word_tokens) <= 1:
            return [], np.zeros(0), np.zeros(0)
        word_boundaries = np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
    else:
        if len(starts) <= 1:
            return [], np.zeros(0), np.zeros(0)
        word_boundaries = starts
        words = None
        if want_words:
            ends = list(starts[1:]) + [len(toks)]
            words = [tokenizer.decode_with_timestamps(toks[a:b]) for a, b in zip(starts, ends)]
    jump_times = np.asarray(jump_frames[:len(toks)], dtype=np.int64) / TOKENS_PER_SECOND
    return words, jump_times[word_boundaries[:-1]], jump_times[word_boundaries[1:]]
