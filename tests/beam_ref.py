"""Beam search as upstream openai-whisper decodes with it -- BeamSearchDecoder.update / finalize and MaximumLikelihoodRanker of decoding.py,
an absent third-party dependency, restated from the published algorithm -- in numpy / float64, as the reference of the GPU beam step
(csrc/beam.hip through wca_test_beam_step and wca_decode_group). Host only: no GPU, no engine.

Where upstream leaves an order open this restatement fixes it, and the engine follows the same rules (include/wca.h, wca_decode_group):
  * a row's top beam_size + 1 log-probabilities: the lower token first among equals (torch.topk promises no order there);
  * the candidates of an audio: score descending, then the lower source beam, then the lower token (upstream sorts a dict whose equal
    scores keep insertion order: source-major, which this is);
  * at the first choice the beams of an audio are identical rows, and upstream's dict keyed by the sequence keeps ONE copy of every
    candidate: only beam 0 offers candidates (first=True);
  * finalize tops a short list up from the live beams in descending sum_logprob, the lower beam first among equals.

Every decision also reports its margin, so that a test can tell a planted exact tie (margin 0, decided by the rules above on both sides)
from a near-tie that fp32 and float64 could decide differently: update() returns the smallest NON-ZERO score gap at its selection
boundaries (each row's cut between the kept and the first dropped log-probability, and every pair of neighbours among the candidates the
walk reached, the first one it did not reach included) and, separately, the number of exact ties it met there.
"""
import numpy as np

GROUP_MIX = 0x94D049BB133111EB


def group_seed(seed, g):
    """decoding.group_seed, restated: sample g of a row with seed `seed` draws with this Philox seed; g = 0 keeps the seed."""
    return (int(seed) ^ (int(g) * GROUP_MIX)) % (1 << 64)


def log_softmax(filtered):
    """float64 log-softmax of one row of filtered logits (-inf = removed)."""
    x = np.asarray(filtered, dtype=np.float64)
    m = x[np.isfinite(x)].max()
    return x - (m + np.log(np.exp(x[np.isfinite(x)] - m).sum()))


def top_candidates(logprobs, k):
    """The k most probable tokens of a row, lowest token first among equals: ([(logprob, token)], gap to the first dropped one)."""
    live = np.nonzero(np.isfinite(logprobs))[0]
    if len(live) > k + 1:   # only what is at least as probable as the (k + 1)-th can be kept or be the first dropped one
        live = live[logprobs[live] >= np.partition(logprobs[live], -(k + 1))[-(k + 1)]]
    order = live[np.lexsort((live, -logprobs[live]))]
    kept = [(float(logprobs[t]), int(t)) for t in order[:k]]
    gap = float(logprobs[order[k - 1]] - logprobs[order[k]]) if len(order) > k else np.inf
    return kept, gap


class BeamSearch:
    def __init__(self, n_audio, beam_size, eot, patience=None):
        self.n_audio, self.beam_size, self.eot = n_audio, beam_size, eot
        self.max_candidates = max(1, round(beam_size * (patience or 1.0)))
        self.finished = [[] for _ in range(n_audio)]   # per audio: [(sequence tuple with its closing eot, score)], in the order they joined

    def update(self, tokens, filtered_logits, sum_logprobs, first=False, frozen=()):
        """tokens: R = n_audio * beam_size token lists; filtered_logits [R, V] (the logit filters already applied: -inf = removed);
        sum_logprobs [R]. frozen: audios past their budget (copied through). Returns (next_tokens, sources [R] absolute source rows,
        new sum_logprobs [R] float64, completed, min_gap, n_ties)."""
        G, eot = self.beam_size, self.eot
        next_tokens, sources, sums = [], [], []
        gaps, ties = [], 0

        def margin(a, b):
            nonlocal ties
            if a == b:
                ties += 1
            else:
                gaps.append(abs(a - b))

        for i in range(self.n_audio):
            if i in frozen:
                for j in range(G):
                    next_tokens.append(list(tokens[i * G + j]))
                    sources.append(i * G + j)
                    sums.append(float(sum_logprobs[i * G + j]))
                continue
            cands = []   # (score, source beam, token)
            for j in range(1 if first else G):
                kept, gap = top_candidates(log_softmax(filtered_logits[i * G + j]), G + 1)
                if np.isfinite(gap):
                    margin(gap, 0.0)
                cands += [(float(sum_logprobs[i * G + j]) + lp, j, t) for lp, t in kept]
            cands.sort(key=lambda c: (-c[0], c[1], c[2]))
            saved, newly, reached = 0, [], 0
            for n, (score, j, t) in enumerate(cands):
                reached = n + 1
                if t == eot:
                    newly.append((tuple(tokens[i * G + j]) + (eot,), score))
                else:
                    next_tokens.append(list(tokens[i * G + j]) + [t])
                    sources.append(i * G + j)
                    sums.append(score)
                    saved += 1
                    if saved == G:
                        break
            assert saved == G, "fewer than beam_size candidates survived the filters"
            for a, b in zip(cands[:reached], cands[1:reached + 1]):
                margin(a[0], b[0])
            for seq, score in newly:   # (already best first)
                if len(self.finished[i]) >= self.max_candidates:
                    break
                self.finished[i].append((seq, score))
        completed = all(len(f) >= self.max_candidates or i in frozen for i, f in enumerate(self.finished))
        return next_tokens, np.array(sources), np.array(sums, dtype=np.float64), completed, (min(gaps) if gaps else np.inf), ties

    def n_done(self, frozen=()):
        return sum(1 for i, f in enumerate(self.finished) if len(f) >= self.max_candidates or i in frozen)

    def finalize(self, tokens, sum_logprobs):
        """Per audio [(sequence with its closing eot, sum_logprob)]: the finished list, topped up to beam_size from the live beams."""
        G, out = self.beam_size, []
        for i, fin in enumerate(self.finished):
            seqs = list(fin)
            if len(seqs) < G:
                order = sorted(range(G), key=lambda j: (-float(sum_logprobs[i * G + j]), j))
                for j in order:
                    seqs.append((tuple(tokens[i * G + j]) + (self.eot,), float(sum_logprobs[i * G + j])))
                    if len(seqs) >= G:
                        break
            out.append(seqs)
        return out


def rank(sum_logprobs, lengths, length_penalty=None):
    """MaximumLikelihoodRanker.rank for one audio: the index of the best sequence (lengths: sampled tokens without the closing eot --
    upstream counts the tokens before it); sum / length, or sum / ((5 + length) / 6) ** length_penalty; the first maximum wins and a
    sequence of length 0 ranks last."""
    def score(s, n):
        if n <= 0:
            return -np.inf
        return float(s) / (float(n) if length_penalty is None else ((5 + n) / 6) ** length_penalty)
    scores = [score(s, n) for s, n in zip(sum_logprobs, lengths)]
    best = 0
    for i, v in enumerate(scores):
        if v > scores[best]:
            best = i
    return best
