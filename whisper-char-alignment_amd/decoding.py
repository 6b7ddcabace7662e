"""Greedy ASR pre-pass: `whisper.decode(model, mel, options)` as the reference calls it (infer_ali.py:40,60-61,
probe_oracle.py:37,59-60, README.md:107-108) on the MI355X engine (C ABI wca_decode).

Upstream openai-whisper `decoding.py` is an absent third-party dependency; its published algorithm is restated here
(host side: which tokens the filters suppress) and in csrc/decode.hip (the per-step filters and GreedyDecoder.update).
Built: language identification (`detect_language`, C ABI wca_detect_language: one decoder position and the language head on the GPU;
the encoded state stays for the decode that follows, so detecting and decoding a window costs ONE encoder pass where upstream runs two),
decode in a given language (DecodingOptions(language=None) is refused: call detect_language first, or transcribe(language="auto")),
temperature 0 greedily or with beam search, and conditioning on a prompt and / or
a prefix (DecodingOptions(prompt=...), the decoder side of transcribe(initial_prompt=...); prefix=...), whose initial tokens
go through the decoder in one batched forward (wca_decode, prefill); a list of options gives every batch row a
prompt / prefix of its own (wca_decode with per_row 1). Temperature sampling is opt-in through the engine-specific
DecodingOptions(seed=<int>): with a seed, temperature > 0 draws every token from softmax(filtered logits / temperature), as
upstream's GreedyDecoder.update does, and avg_logprob sums the untempered log-probabilities (wca_decode with temperature_host / seed_host; the rows of
a list may differ in temperature and seed as well). The draw is Gumbel-max over Philox4x32-10 noise in the decode step's kernel
(csrc/decode.hip): the law is upstream's, the draws are not torch's, because the generator differs; it is pinned token for token
against a float64 restatement (tests/decode_sample_ref.py). With seed=None a temperature other than 0 raises as it always did.
Beam search and best_of (C ABI wca_decode_group; csrc/beam.hip): DecodingOptions(beam_size=G [, patience]) at temperature 0 is upstream's
BeamSearchDecoder on G decoder rows per audio that share the audio's cross-K/V, DecodingOptions(best_of=G, temperature > 0, seed) is G
independent samples per audio (sample g drawing with group_seed(seed, g)), and MaximumLikelihoodRanker (length_penalty) picks the result on
the host; rows x G must fit the engine's max_batch. Pinned against a float64 restatement of upstream's update / finalize / ranker
(tests/beam_ref.py) and against the fp32 oracle replayed along the engine's beams; where upstream leaves an order open (equal logits in
topk, equal scores) the order is fixed here: lower source beam, then lower token. Upstream's own option checks raise its ValueErrors.
Anything else raises NotImplementedError instead of silently differing.
PARITY UNPINNED against upstream itself for decode and detect_language alike (no real checkpoint is at hand): both are pinned
against this repository's fp32 CPU oracle on synthetic weights.
"""
import dataclasses
import zlib
from dataclasses import dataclass, field
from typing import List, Optional, Union

import numpy as np
import torch

from . import _lib
from .tokenizer import get_tokenizer

CHUNK_LENGTH = 30


@dataclass(frozen=True)
class DecodingOptions:
    task: str = "transcribe"
    language: Optional[str] = None
    temperature: float = 0.0
    sample_len: Optional[int] = None
    best_of: Optional[int] = None
    beam_size: Optional[int] = None
    patience: Optional[float] = None
    length_penalty: Optional[float] = None
    prompt: Optional[Union[str, List[int]]] = None
    prefix: Optional[Union[str, List[int]]] = None
    suppress_tokens: Optional[Union[str, tuple]] = "-1"
    suppress_blank: bool = True
    without_timestamps: bool = False
    max_initial_timestamp: Optional[float] = 1.0
    fp16: bool = True
    vocab_path: Optional[str] = None  # engine-specific: local tiktoken file for the tokenizer
    seed: Optional[int] = None        # engine-specific: an int allows temperature > 0 (the engine's sampling is reproducible by
                                      # construction and picks no seed for the caller); over a batch, row b draws with seed + b


@dataclass(frozen=True)
class DecodingResult:
    language: str
    tokens: List[int] = field(default_factory=list)
    text: str = ""
    avg_logprob: float = np.nan
    no_speech_prob: float = np.nan
    temperature: float = np.nan
    compression_ratio: float = np.nan


def compression_ratio(text):
    text_bytes = text.encode("utf-8")
    return len(text_bytes) / len(zlib.compress(text_bytes))


def suppress_token_ids(tokenizer, options):
    """DecodingTask._get_suppress_tokens (upstream, restated): "-1" expands to the non-speech tokens; the task /
    sot / prev / lm / no-speech specials are always suppressed."""
    suppress = options.suppress_tokens
    if isinstance(suppress, str):
        suppress = [int(t) for t in suppress.split(",")]
    suppress = list(suppress) if suppress is not None else []
    if -1 in suppress:
        suppress = [t for t in suppress if t >= 0]
        suppress.extend(tokenizer.non_speech_tokens)
    elif len(suppress) == 0:
        suppress = []
    suppress.extend([tokenizer.transcribe, tokenizer.translate, tokenizer.sot, tokenizer.sot_prev, tokenizer.sot_lm])
    if tokenizer.no_speech is not None:
        suppress.append(tokenizer.no_speech)
    return tuple(sorted(set(suppress)))


def filter_masks(tokenizer, options, n_vocab):
    """(suppress_mask, blank_mask) byte arrays [n_vocab] for wca_decode."""
    sup = np.zeros(n_vocab, dtype=np.uint8)
    if options.suppress_tokens:
        ids = [t for t in suppress_token_ids(tokenizer, options) if t < n_vocab]
        sup[ids] = 1
    if not options.without_timestamps and tokenizer.no_timestamps is not None and tokenizer.no_timestamps < n_vocab:
        sup[tokenizer.no_timestamps] = 1  # ApplyTimestampRules suppresses <|notimestamps|>
    blank = None
    if options.suppress_blank:
        blank = np.zeros(n_vocab, dtype=np.uint8)
        blank[[t for t in tokenizer.encode(" ") + [tokenizer.eot] if t < n_vocab]] = 1
    return sup, blank


GROUP_MAX = 16                   # decoder rows per audio (BEAM_GROUP_MAX of the library)
GROUP_MIX = 0x94D049BB133111EB   # odd: distinct g give distinct seeds


def group_seed(seed, g):
    """The Philox seed of sample g of a row whose seed is `seed` (best_of; include/wca.h, wca_decode_group): the row's seed mixed with the
    sample's index, so that sample 0 is the plain sampled decode of that seed and a row's samples do not depend on the batch it rides in."""
    return (int(seed) ^ (int(g) * GROUP_MIX)) % (1 << 64)


def sequence_score(sum_logprob, length, length_penalty=None):
    """MaximumLikelihoodRanker's score of one sequence (upstream, restated): sum_logprob / length, or with a length penalty
    sum_logprob / ((5 + length) / 6) ** length_penalty (Google NMT). A sequence without sampled tokens scores -inf: it ranks last."""
    if length <= 0:
        return -np.inf
    penalty = float(length) if length_penalty is None else ((5 + length) / 6) ** length_penalty
    return float(sum_logprob) / penalty


def rank_sequences(sum_logprobs, lengths, length_penalty=None):
    """MaximumLikelihoodRanker.rank for one audio: the index of the best sequence, the first among equal scores."""
    scores = [sequence_score(s, n, length_penalty) for s, n in zip(sum_logprobs, lengths)]
    return int(np.argmax(scores))


def _check_supported(options, grouped=False):
    """What is refused instead of silently differing from upstream. grouped: the caller can give every audio several decoder rows (decode()
    does, through wca_decode_group); only then are beam_size / patience / best_of taken, under upstream's own checks
    (DecodingTask._verify_options). A check on behalf of a plain one-row-per-audio decode refuses them as it always did."""
    sampling = options.temperature != 0.0 and options.seed is not None   # opt-in: without a seed every refusal is what it was
    if sampling and not (isinstance(options.temperature, (int, float)) and 0.0 <= options.temperature < float("inf")):
        raise ValueError("temperature must be a finite number >= 0, not %r" % (options.temperature,))
    if options.seed is not None and (isinstance(options.seed, bool) or not isinstance(options.seed, (int, np.integer))):
        raise ValueError("seed must be an int (or None: temperature 0 only), not %r" % (options.seed,))
    if options.temperature != 0.0 and not sampling:
        raise NotImplementedError("temperature %r needs DecodingOptions(seed=<int>): the engine's sampling (and with it best_of) is reproducible "
                                  "by construction and picks no seed for the caller; without one only temperature 0 is decoded" % (options.temperature,))
    if not grouped and (options.beam_size is not None or options.best_of is not None or options.patience is not None):
        raise NotImplementedError("beam_size / patience / best_of take several decoder rows per audio: decode() runs them (C ABI "
                                  "wca_decode_group); a decode of one row per audio does not")
    for name in ("beam_size", "best_of"):
        v = getattr(options, name)
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= GROUP_MAX):
            raise ValueError("%s must be an int in [1, %d], not %r" % (name, GROUP_MAX, v))
    if options.beam_size is not None and options.best_of is not None:
        raise ValueError("beam_size and best_of can't be given together")
    if options.patience is not None and (options.beam_size is None or not options.patience > 0):
        raise ValueError("patience requires beam_size to be given, and must be positive")
    if options.length_penalty is not None and not 0 <= options.length_penalty <= 1:
        raise ValueError("length_penalty (alpha) should be a value between 0 and 1")
    if options.temperature == 0.0 and options.best_of is not None:
        raise ValueError("best_of with greedy sampling (T=0) is not compatible")
    if options.temperature != 0.0 and options.beam_size is not None:
        raise ValueError("beam_size needs temperature 0 (upstream's fallback drops it on the rungs above 0: pass best_of there)")
    if options.language is None:
        raise NotImplementedError("decode takes a given language: pass DecodingOptions(language=...) as infer_ali.py:40 does; "
                                  "detect_language(model, mel) names it, and transcribe(language=\"auto\") does both")


def _text_tokens(tokenizer, text, options, what):
    if isinstance(text, str):
        if options.vocab_path is None:
            raise ValueError("a str %s is BPE-encoded and needs the vocabulary: pass DecodingOptions(vocab_path=<local *.tiktoken "
                             "file>), or give the %s as a list of token ids" % (what, what))
        return tokenizer.encode(" " + text.strip())
    return [int(t) for t in text]


def initial_tokens(tokenizer, options, n_ctx, sample_len):
    """DecodingTask._get_initial_tokens (upstream, restated): [sot_prev, prompt[-(n_ctx // 2 - 1):]] + sot_sequence
    [+ no_timestamps] + prefix[-(n_ctx // 2 - sample_len):] (Python slicing as upstream: a 0 bound keeps the whole prefix,
    a negative one drops tokens from its front)."""
    tokens = list(tokenizer.sot_sequence_including_notimestamps if options.without_timestamps else tokenizer.sot_sequence)
    if options.prefix:
        prefix_tokens = _text_tokens(tokenizer, options.prefix, options, "prefix")
        if sample_len is not None:
            max_prefix_len = n_ctx // 2 - sample_len
            prefix_tokens = prefix_tokens[-max_prefix_len:]
        tokens = tokens + prefix_tokens
    if options.prompt:
        prompt_tokens = _text_tokens(tokenizer, options.prompt, options, "prompt")
        tokens = [tokenizer.sot_prev] + prompt_tokens[-(n_ctx // 2 - 1):] + tokens
    return tokens


def decode_plan(tokenizer, options, n_ctx):
    """(initial tokens, sample_len as run, sot_index): upstream's loop stops after sample_len steps or once the sequence is
    longer than n_ctx, so at most min(sample_len, n_ctx + 1 - len(initial)) tokens are sampled."""
    sample_len = options.sample_len or n_ctx // 2
    initial = initial_tokens(tokenizer, options, n_ctx, sample_len)
    if len(initial) > n_ctx:
        raise ValueError("the prompt and prefix give %d initial tokens, more than n_text_ctx = %d: nothing can be decoded" % (len(initial), n_ctx))
    return initial, min(sample_len, n_ctx + 1 - len(initial)), initial.index(tokenizer.sot)


@torch.no_grad()
def detect_language(model, mel, tokenizer=None, *, pcm=None, n_samples=None):
    """whisper.detect_language(model, mel, tokenizer) -> (language_tokens, language_probs): the most probable language token of
    every row ([B] int64 tensor) and one {language code: probability} dict per row; a [n_mels, 3000] mel gives a 0-dim tensor and
    one dict. mel: f32 cuda tensor, or None with pcm [B, stride] f32 cuda + n_samples (the log-mel then runs on the device).
    The default tokenizer numbers model.num_languages languages, as upstream. A model without language tokens (English-only)
    raises upstream's ValueError. The encoded state stays in the engine: decode(model, None, options, encoded_batch=B) right after
    decodes these rows with no second encoder pass."""
    if tokenizer is None:
        tokenizer = get_tokenizer(model.is_multilingual, num_languages=model.num_languages)
    if tokenizer.language is None or tokenizer.language_token not in tokenizer.sot_sequence:
        raise ValueError("This model doesn't have language tokens so it can't perform lang id")
    single = mel is not None and mel.ndim == 2
    if single:
        mel = mel.unsqueeze(0)
    lang_tokens, codes = tokenizer.all_language_tokens, tokenizer.all_language_codes
    if list(lang_tokens) != list(range(lang_tokens[0], lang_tokens[0] + len(lang_tokens))):
        raise ValueError("the tokenizer's language tokens are not one contiguous id range")
    tokens, probs = model.detect_language(mel, pcm=pcm, n_samples=n_samples, sot=tokenizer.sot, lang_begin=lang_tokens[0], n_lang=len(lang_tokens))
    language_tokens = torch.from_numpy(np.asarray(tokens, dtype=np.int64))
    language_probs = [{c: float(p) for c, p in zip(codes, row)} for row in probs]
    if single:
        return language_tokens[0], language_probs[0]
    return language_tokens, language_probs


@torch.no_grad()
def decode(model, mel, options=DecodingOptions(), pcm=None, n_samples=None, encoded_batch=None, want_text=True, redecode=False,
           row_sample_len=None):
    """whisper.decode. mel: [n_mels, 3000] or [B, n_mels, 3000] f32 cuda tensor (or None with pcm [B, stride] f32 cuda +
    n_samples, the log-mel then runs on the device; or neither with encoded_batch=B: decode the state queued by
    model.encode_batch). Returns DecodingResult or a list of them. want_text=False (transcribe without a vocabulary file) leaves
    `text` empty instead of decoding the token ids, which only the BPE vocabulary can do.
    options may also be a list with one DecodingOptions per batch row; the rows may differ in prompt / prefix / temperature / seed only
    (ValueError otherwise): they then sit at different decoder positions (wca_decode with per_row 1) and the result is always a list.
    Sampling is opt-in through DecodingOptions(seed=<int>): temperature > 0 then draws every token from softmax(filtered logits /
    temperature) as upstream's GreedyDecoder does, avg_logprob from the untempered log-probabilities (wca_decode with temperature_host / seed_host: Gumbel-max
    over Philox noise -- upstream's law, not torch's draws). One DecodingOptions over B rows gives row b the seed (seed + b) mod 2^64; a
    list gives every row its own. A row at temperature 0 is decoded greedily whatever its seed, and a call whose rows are all at
    temperature 0 is exactly the greedy engine call.
    redecode=True (mel = pcm = None, encoded_batch=B): decode AGAIN the state that the previous decode of these B rows left for the
    alignment, with no encoder pass (the rungs of transcribe's temperature fallback); the state stays for align_batch(pcm=None).
    row_sample_len (with a list of options; one int or None per row) caps a row's sampled tokens below its options' sample_len: the rows
    of a re-decode whose first result was kept ride along for one token."""
    per_row = isinstance(options, (list, tuple))
    rows = list(options) if per_row else [options]
    if not rows:
        raise ValueError("an empty list of DecodingOptions")
    for o in rows:
        _check_supported(o, grouped=True)
    if any((o.beam_size, o.patience) != (rows[0].beam_size, rows[0].patience) for o in rows):
        raise NotImplementedError("the rows of one decode share beam_size and patience: a decode whose audios take different numbers of "
                                  "decoder rows is not built")
    common = [dataclasses.replace(o, prompt=None, prefix=None, temperature=0.0, seed=None, best_of=None) for o in rows]
    for b, c in enumerate(common):
        if c != common[0]:
            diff = [f.name for f in dataclasses.fields(c) if getattr(c, f.name) != getattr(common[0], f.name)]
            raise ValueError("the rows of one decode may differ in prompt / prefix / temperature / seed only; row %d differs from row 0 in %s"
                             % (b, ", ".join(diff)))
    best_of = {o.best_of for o in rows if o.temperature != 0.0}   # (a row at temperature 0 carries none: it rides along greedily)
    if len(best_of) > 1:
        raise ValueError("the rows of one decode that sit at a temperature above 0 must share best_of")
    best_of, beam_size = (best_of.pop() if best_of else None), rows[0].beam_size
    if redecode and (mel is not None or pcm is not None or encoded_batch is None):
        raise ValueError("redecode=True decodes the state of the previous decode again: pass mel = pcm = None and encoded_batch=B")
    single = mel is not None and mel.ndim == 2
    if single:
        mel = mel.unsqueeze(0)
    B = mel.shape[0] if mel is not None else (pcm.shape[0] if pcm is not None else int(encoded_batch))
    if per_row and len(rows) != B:
        raise ValueError("%d DecodingOptions for a batch of %d" % (len(rows), B))
    first, dims = rows[0], model.dims
    tokenizer = get_tokenizer(model.is_multilingual, language=first.language, task=first.task, vocab_path=first.vocab_path)
    plans = [decode_plan(tokenizer, o, dims.n_text_ctx) for o in rows]   # (initial tokens, sample_len, sot_index) per row
    if row_sample_len is not None:
        if not per_row or len(row_sample_len) != B:
            raise ValueError("row_sample_len takes one entry per row of a list of DecodingOptions")
        plans = [(p[0], p[1] if cap is None else max(1, min(p[1], int(cap))), p[2]) for p, cap in zip(plans, row_sample_len)]
    sup, blank = filter_masks(tokenizer, first, dims.n_vocab)
    max_init = -1
    if not first.without_timestamps and first.max_initial_timestamp is not None:
        max_init = round(first.max_initial_timestamp / (CHUNK_LENGTH / dims.n_audio_ctx))
    kw = dict(eot=tokenizer.eot, timestamp_begin=tokenizer.timestamp_begin, apply_timestamp_rules=not first.without_timestamps,
              max_initial_timestamp_index=max_init, batch=B, no_speech=tokenizer.no_speech if tokenizer.no_speech is not None else -1)
    grouped, sampling = beam_size is not None or best_of is not None, redecode or any(o.temperature != 0.0 for o in rows)
    if not per_row and (grouped or sampling):   # one DecodingOptions over the batch: row b draws with seed + b
        rows, plans = [dataclasses.replace(first, seed=None if first.seed is None else int(first.seed) + b) for b in range(B)], plans * B
    row_arrays = ([p[0] for p in plans], [p[2] for p in plans], [p[1] for p in plans])   # initial tokens, sot_index, sample_len per row
    sampled = dict(temperature=[float(o.temperature) for o in rows], seed=[int(o.seed or 0) % (1 << 64) for o in rows])
    if grouped:
        # G decoder rows per audio (wca_decode_group): the beams, or best_of independent samples; then upstream's MaximumLikelihoodRanker
        G = beam_size if beam_size is not None else best_of
        if B * G > getattr(model, "max_batch", B * G):
            raise NotImplementedError("%d audios x %d decoder rows each exceed the engine's max_batch = %d, and a group is not split over "
                                      "several calls: create the engine with more rows" % (B, G, model.max_batch))
        slots, n_slots, sums, n_out = model.decode_group(mel, pcm, n_samples, *row_arrays, sup, blank, redecode=redecode, n_group=G,
                                                         mode=0 if beam_size is not None else 1,
                                                         max_candidates=max(1, round(G * (first.patience or 1.0))) if beam_size is not None else None,
                                                         **(sampled if beam_size is None else {}), **kw)
        best = [rank_sequences(sums[b, :n_out[b]], n_slots[b, :n_out[b]] - len(plans[b][0]), first.length_penalty) for b in range(B)]
        tokens = np.stack([slots[b, i] for b, i in enumerate(best)])
        n_tokens, sum_logprobs = [n_slots[b, i] for b, i in enumerate(best)], [sums[b, i] for b, i in enumerate(best)]
    elif sampling:
        tokens, n_tokens, sum_logprobs = model.decode_rows_sampled(mel, pcm, n_samples, *row_arrays, sup, blank, redecode=redecode, **sampled, **kw)
    elif per_row:
        tokens, n_tokens, sum_logprobs = model.greedy_decode_rows(mel, pcm, n_samples, *row_arrays, sup, blank, **kw)
    else:
        initial, sample_len, sot_index = plans[0]
        tokens, n_tokens, sum_logprobs = model.greedy_decode(mel, pcm, n_samples, initial, sup, blank, sample_len=sample_len, sot_index=sot_index,
                                                             prefill=1 if first.prompt or first.prefix else 0, **kw)
        plans = plans * B
    rows = rows if len(rows) == B else rows * B
    no_speech_probs = model.last_no_speech_prob
    results = []
    for b in range(B):
        toks = [int(t) for t in tokens[b, len(plans[b][0]):n_tokens[b]]]
        text = tokenizer.decode(toks).strip() if want_text else ""
        results.append(DecodingResult(language=first.language, tokens=toks, text=text, avg_logprob=float(sum_logprobs[b]) / (len(toks) + 1),
                                      no_speech_prob=float(no_speech_probs[b]), temperature=rows[b].temperature,
                                      compression_ratio=compression_ratio(text) if text else np.nan))
    return results[0] if single and not per_row else results
