"""`import timing` drop-in for the reference's timing.py (timing.py:13-186): the same four functions, running on the
MI355X engine. Put this directory on sys.path instead of the reference checkout."""
from _pkg import sub as _sub

_t = _sub("timing")
filter_attention = _t.filter_attention
get_attentions = _t.get_attentions
force_align = _t.force_align
default_find_alignment = _t.default_find_alignment
median_filter = _t.median_filter
dtw = _t.dtw
dtw_open = _t.dtw_open
dtw_windows = _t.dtw_windows
path_scores = _t.path_scores
word_alignment_scores = _t.word_alignment_scores
force_align_long = _t.force_align_long
force_align_long_batch = _t.force_align_long_batch
force_align_cues = _t.force_align_cues
force_align_cues_batch = _t.force_align_cues_batch
trim_words_to_speech = _t.trim_words_to_speech
HOP_LENGTH, SAMPLE_RATE, TOKENS_PER_SECOND = _t.HOP_LENGTH, _t.SAMPLE_RATE, _t.TOKENS_PER_SECOND
