"""Model handle of the MI355X engine: the object callers pass as `model` to timing.get_attentions
(reference: `whisper.load_model(...)` at infer_ali.py:36 / README.md:93).

It exposes the attributes the reference's callers touch (`model.device`, `model.dims.n_text_layer`,
`model.is_multilingual`; infer_ali.py:41,46, timing.py:48) and owns one `wca_engine` (weights in HBM as
f16, activation arena, HIP stream). PyTorch-ROCm is used only to hold device buffers and to read
checkpoints; all arithmetic happens in libwca.so.
"""
import ctypes as C
from dataclasses import dataclass, asdict

import numpy as np
import torch

from . import _lib
from .audio import mel_filters

N_FRAMES = 3000
N_SAMPLES = 480000
MAX_FRAMES = 1500   # infer_ali.py:25
MAX_LENGTH = 448    # infer_ali.py:26
_pf32, _pi32 = C.POINTER(C.c_float), C.POINTER(C.c_int32)


@dataclass
class ModelDimensions:
    """Same fields as whisper.model.ModelDimensions."""
    n_mels: int
    n_audio_ctx: int
    n_audio_state: int
    n_audio_head: int
    n_audio_layer: int
    n_vocab: int
    n_text_ctx: int
    n_text_state: int
    n_text_head: int
    n_text_layer: int


# whisper model sizes
_SIZES = {
    "tiny": (384, 6, 4), "base": (512, 8, 6), "small": (768, 12, 12), "medium": (1024, 16, 24),
    "large": (1280, 20, 32), "large-v1": (1280, 20, 32), "large-v2": (1280, 20, 32), "large-v3": (1280, 20, 32),
}


def dims_for(name):
    """ModelDimensions for an official model name ('medium', 'tiny.en', 'large-v3', ...)."""
    base = name[:-3] if name.endswith(".en") else name
    if base not in _SIZES:
        raise ValueError("unknown whisper model %r" % name)
    d, h, l = _SIZES[base]
    multilingual = not name.endswith(".en")
    n_mels = 128 if base == "large-v3" else 80
    n_vocab = 51866 if base == "large-v3" else (51865 if multilingual else 51864)
    return ModelDimensions(n_mels, 1500, d, h, l, n_vocab, 448, d, h, l)


# openai-whisper's per-model alignment heads (`whisper._ALIGNMENT_HEADS`, applied by whisper.load_model(name) through
# set_alignment_heads): the (layer, head) pairs of the decoder cross-attention heads highly correlated with word timing.
# Published data of the upstream package, kept here in BOTH forms: the package's own base85 + gzip boolean masks
# (ALIGNMENT_HEADS_B85, decoded by decode_alignment_heads exactly like whisper.model.Whisper.set_alignment_heads:
# b85decode -> gzip -> bool[n_text_layer, n_text_head]) and the decoded index lists, row-major like
# `model.alignment_heads.indices().T` (timing.py:155). tests/test_host.py decodes every mask (the gzip CRC-32 validates each
# string byte for byte) and requires it to equal the list below.
ALIGNMENT_HEADS_B85 = {
    "tiny.en": b"ABzY8J1N>@0{>%R00Bk>$p{7v037`oCl~+#00",
    "tiny": b"ABzY8bu8Lr0{>%RKn9Fp%m@SkK7Kt=7ytkO",
    "base.en": b"ABzY8;40c<0{>%RzzG;p*o+Vo09|#PsxSZm00",
    "base": b"ABzY8KQ!870{>%RzyTQH3`Q^yNP!>##QT-<FaQ7m",
    "small.en": b"ABzY8>?_)10{>%RpeA61k&I|OI3I$65C{;;pbCHh0B{qLQ;+}v00",
    "small": b"ABzY8DmU8=0{>%Rpa?J`kvJ6qF(V^F86#Xh7JUGMK}P<N0000",
    "medium.en": b"ABzY8usPae0{>%R7<zz_OvQ{)4kMa0BMw6u5rT}kRKX;$NfYBv00*Hl@qhsU00",
    "medium": b"ABzY8B0Jh+0{>%R7}kK1fFL7w6%<-Pf*t^=N)Qr&0RR9",
    "large-v1": b"ABzY8r9j$a0{>%R7#4sLmoOs{s)o3~84-RPdcFk!JR<kSfC2yj",
    "large-v2": b"ABzY8zd+h!0{>%R7=D0pU<_bnWW*tkYAhobTNnu$jnkEkXqp)j;w1Tzk)UH3X%SZd&fFZ2fC2yj",
    "large-v3": b"ABzY8gWO1E0{>%R7(9S+Kn!D~%ngiGaR?*L!iJG9p-nab0JQ=-{D1-g00",
}


def decode_alignment_heads(dump, n_text_layer, n_text_head):
    """base85 + gzip boolean mask -> [(layer, head), ...] in row-major order (whisper.model.Whisper.set_alignment_heads)."""
    import base64
    import gzip
    mask = np.frombuffer(gzip.decompress(base64.b85decode(dump)), dtype=bool).reshape(n_text_layer, n_text_head)
    return [(int(l), int(h)) for l, h in np.argwhere(mask)]


ALIGNMENT_HEADS = {
    "tiny.en": [(1, 0), (2, 0), (2, 5), (3, 0), (3, 1), (3, 2), (3, 3), (3, 4)],
    "tiny": [(2, 2), (3, 0), (3, 2), (3, 3), (3, 4), (3, 5)],
    "base.en": [(3, 3), (4, 7), (5, 1), (5, 5), (5, 7)],
    "base": [(3, 1), (4, 2), (4, 3), (4, 7), (5, 1), (5, 2), (5, 4), (5, 6)],
    "small.en": [(6, 6), (7, 0), (7, 3), (7, 8), (8, 2), (8, 5), (8, 7), (9, 0), (9, 4), (9, 8), (9, 10), (10, 0), (10, 1), (10, 2),
                 (10, 3), (10, 6), (10, 11), (11, 2), (11, 4)],
    "small": [(5, 3), (5, 9), (8, 0), (8, 4), (8, 7), (8, 8), (9, 0), (9, 7), (9, 9), (10, 5)],
    "medium.en": [(11, 4), (14, 1), (14, 12), (14, 14), (15, 4), (16, 0), (16, 4), (16, 9), (17, 12), (17, 14), (18, 7), (18, 10),
                  (18, 15), (20, 0), (20, 3), (20, 9), (20, 14), (21, 12)],
    "medium": [(13, 15), (15, 4), (15, 15), (16, 1), (20, 0), (23, 4)],
    "large-v1": [(9, 19), (11, 2), (11, 4), (11, 17), (22, 7), (22, 11), (22, 17), (23, 2), (23, 15)],
    "large-v2": [(10, 12), (13, 17), (16, 11), (16, 12), (16, 13), (17, 15), (17, 16), (18, 4), (18, 11), (18, 19), (19, 11), (21, 2),
                 (21, 3), (22, 3), (22, 9), (22, 12), (23, 5), (23, 7), (23, 13), (25, 5), (26, 1), (26, 12), (27, 15)],
    "large-v3": [(7, 0), (10, 17), (12, 18), (13, 12), (16, 1), (17, 14), (19, 11), (21, 4), (24, 1), (25, 6)],
}
ALIGNMENT_HEADS["large"] = ALIGNMENT_HEADS["large-v3"]


def model_name_from_dims(dims):
    """The official model name a set of dimensions identifies, or None when it is ambiguous (large-v1 / large-v2 share
    every dimension) or not an official size."""
    for base, (d, h, l) in _SIZES.items():
        if (dims.n_text_state, dims.n_text_head, dims.n_text_layer) != (d, h, l) or base in ("large", "large-v1", "large-v2", "large-v3"):
            continue
        return base if dims.n_vocab >= 51865 else base + ".en"
    if (dims.n_text_state, dims.n_text_head, dims.n_text_layer) == _SIZES["large"] and dims.n_mels == 128:
        return "large-v3"
    return None


_registry = {}   # device index -> weakref of the most recently constructed engine
_utility = {}    # device index -> weight-less engine created on demand for filter_attention / force_align / dtw


def default_engine(device_index=0, need_weights=False):
    """Most recent live engine on the device; if none exists a tiny weight-less utility engine is
    created (enough for the ops that take no model argument in the reference API)."""
    ref = _registry.get(device_index)
    eng = ref() if ref is not None else None
    if eng is not None and (eng._finalized or not need_weights):
        return eng
    if need_weights:
        raise RuntimeError("no WhisperAMD engine with weights exists on cuda:%d" % device_index)
    if device_index not in _utility:
        _utility[device_index] = WhisperAMD(ModelDimensions(80, 1500, 128, 2, 1, 51865, 448, 128, 2, 1),
                                            device="cuda:%d" % device_index, max_batch=1, _register=False, precision="f16")   # (runs no forward)
    return _utility[device_index]


def _ptr(t):
    """The address of a torch tensor, a numpy array or a ctypes array as a c_void_p; None is the null pointer."""
    if t is None:
        return C.c_void_p(0)
    if hasattr(t, "data_ptr"):
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(t.ctypes.data if hasattr(t, "ctypes") else C.addressof(t))


def _batch_size(mel, pcm, batch):
    """The rows of a call that takes mel XOR pcm, or neither with batch=B (a state queued by encode_batch or left by the last decode)."""
    return mel.shape[0] if mel is not None else (pcm.shape[0] if pcm is not None else int(batch))


def _temps_seeds(B, temperature, seed):
    """One temperature (float >= 0) and one seed (int, taken mod 2^64) per row, as the arrays wca_decode_desc points to."""
    if temperature is None or seed is None or len(temperature) != B or len(seed) != B:
        raise ValueError("temperature and seed take one entry per batch row (%d)" % B)
    return (np.ascontiguousarray([float(t) for t in temperature], dtype=np.float32),
            np.ascontiguousarray([int(v) % (1 << 64) for v in seed], dtype=np.uint64))


class WhisperAMD:
    def __init__(self, dims, device="cuda:0", max_batch=8, _register=True, precision="reference"):
        """precision: 'reference' (default since round 5, like wca_engine_create): the CONTRACT mode -- the reference's fp32 forward
        (/root/reference/timing.py:58) to fp32 summation noise; 'f16': the fast single-f16-operand mode (98.5 % of the word boundaries
        within one frame on the parity legs) as an explicit opt-in. set_precision() switches later."""
        if precision not in ("reference", "split", "f16"):
            raise ValueError("precision must be 'reference' (= 'split') or 'f16'")
        if not torch.cuda.is_available():
            raise RuntimeError("WhisperAMD needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self._lib = _lib.load()
        self.dims = dims
        self.device = torch.device(device)
        self.max_batch = int(max_batch)
        self._h = C.c_void_p(0)
        cd = _lib.ModelDims(**asdict(dims))
        index = self.device.index if self.device.index is not None else 0
        _lib.check(self._lib.wca_engine_create_ex(C.byref(cd), index, self.max_batch, 0 if precision == "f16" else 1, C.byref(self._h)))
        self._stream_bound = None
        self._finalized = False
        # whisper.model.Whisper default: every head of the upper half of the decoder layers; whisper.load_model(name)
        # replaces it with the model's curated heads (ALIGNMENT_HEADS) -- from_checkpoint / use_official_alignment_heads
        self.alignment_heads = [(l, h) for l in range(dims.n_text_layer // 2, dims.n_text_layer) for h in range(dims.n_text_head)]
        self.alignment_heads_source = "default (upper half of the decoder layers)"
        filt = np.ascontiguousarray(mel_filters(dims.n_mels), dtype=np.float32)
        self._load_one("mel_filters", filt)
        if _register:
            import weakref
            _registry[index] = weakref.ref(self)

    # ---- whisper.model.Whisper-like attributes
    @property
    def is_multilingual(self):
        return self.dims.n_vocab >= 51865

    @property
    def num_languages(self):
        return self.dims.n_vocab - 51765 - int(self.is_multilingual)

    def set_alignment_heads(self, heads):
        """heads: iterable of (layer, head) pairs used by timing.default_find_alignment."""
        heads = sorted({(int(l), int(h)) for l, h in heads})  # row-major like alignment_heads.indices().T (timing.py:155)
        for l, h in heads:
            if not (0 <= l < self.dims.n_text_layer and 0 <= h < self.dims.n_text_head):
                raise ValueError("alignment head (%d, %d) out of range" % (l, h))
        self.alignment_heads = heads
        self.alignment_heads_source = "set_alignment_heads"

    def use_official_alignment_heads(self, name=None):
        """What whisper.load_model(name) does after loading the weights: install the model's curated alignment heads.
        `name` defaults to the official model the dimensions identify; returns the name used, or None (with a warning)
        when there is no table for it -- default_find_alignment then averages the generic default set, which is NOT what
        the reference's baseline uses."""
        name = name or model_name_from_dims(self.dims)
        heads = ALIGNMENT_HEADS.get(name)
        if heads is not None and all(l < self.dims.n_text_layer and h < self.dims.n_text_head for l, h in heads):
            self.set_alignment_heads(heads)
            self.alignment_heads_source = "openai-whisper _ALIGNMENT_HEADS[%r]" % name
            return name
        import warnings
        warnings.warn("no official alignment heads for %r with these dimensions: default_find_alignment will use the generic "
                      "default (every head of the upper decoder half); pass the model name (e.g. 'large-v2') or call "
                      "set_alignment_heads" % (name,))
        return None

    def to(self, device):
        if torch.device(device) != self.device:
            raise ValueError("a WhisperAMD engine is bound to %s at construction" % self.device)
        return self

    def eval(self):
        return self

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                self._lib.wca_engine_destroy(self._h)
                self._h = C.c_void_p(0)
        except Exception:
            pass

    # ---- weights
    def _load_one(self, name, arr):
        if isinstance(arr, torch.Tensor):
            arr = arr.detach().cpu()
            if arr.dtype == torch.float16:
                arr = arr.contiguous().numpy()
            else:
                arr = arr.float().contiguous().numpy()
        arr = np.ascontiguousarray(arr)
        if arr.dtype == np.float16:
            dt = _lib.DTYPE_F16
        else:
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            dt = _lib.DTYPE_F32
        shape = (C.c_int64 * max(arr.ndim, 1))(*(arr.shape if arr.ndim else (1,)))
        _lib.check(self._lib.wca_load_weight(self._h, name.encode(), arr.ctypes.data_as(C.c_void_p), dt, shape, max(arr.ndim, 1)))

    def load_state_dict(self, sd, allow_rounded_weights=False):
        """sd: openai-whisper naming (encoder.blocks.0.attn.query.weight ...), torch tensors or numpy arrays.
        Weight matrices are stored f16 (every openai checkpoint is f16 at rest; whisper.load_model upcasts those values,
        /root/reference/infer_ali.py:36-37). An fp32 state dict whose values are NOT f16-representable (a fine-tuned fp32 checkpoint, which the
        reference runs in true fp32) keeps the remainders f16(w - f16(w)) in a second slab and the contract mode multiplies the extra term
        A_hi W_lo^T -- the same hi + lo representation the activations travel in; slower (one more f16 pass per affected GEMM), never narrower.
        allow_rounded_weights=True skips that term (the engine then computes what the f16-ROUNDED checkpoint computes). `weights_inexact` reports
        what was not exact; the f16 mode ignores the remainders (it is approximate by definition)."""
        _lib.check(self._lib.wca_set_allow_rounded_weights(self._h, 1 if allow_rounded_weights else 0))
        for name, t in sd.items():
            self._load_one(name, t)
        _lib.check(self._lib.wca_finalize_weights(self._h))
        self._finalized = True
        return self

    @property
    def weights_inexact(self):
        """(tensors, values, name of the first tensor) whose fp32 source values the f16 weight storage rounded; (0, 0, '') for f16 checkpoints."""
        nt, nv = C.c_longlong(0), C.c_longlong(0)
        buf = C.create_string_buffer(160)
        _lib.check(self._lib.wca_weights_inexact(self._h, C.byref(nt), C.byref(nv), buf, 160))
        return int(nt.value), int(nv.value), buf.value.decode()

    @classmethod
    def from_checkpoint(cls, path, device="cuda:0", max_batch=8, name=None, precision="reference", allow_rounded_weights=False):
        """Loads an openai-format checkpoint ({'dims':..., 'model_state_dict':...}) from a LOCAL path and, like
        whisper.load_model(name), installs the official alignment heads of `name` (inferred from the dimensions when
        they identify the model; large-v1 / large-v2 need the name). This is the drop-in's `whisper.load_model`: the model comes
        back in the CONTRACT precision mode ('reference': the fp32 forward of timing.py:58 to fp32 summation noise), like a bare
        WhisperAMD(); precision='f16' opts out. A checkpoint whose fp32 weights are not f16-representable runs with its remainder slab
        (load_state_dict); allow_rounded_weights=True drops the remainders."""
        ck = torch.load(path, map_location="cpu")
        dims = ModelDimensions(**ck["dims"])
        m = cls(dims, device=device, max_batch=max_batch, precision=precision)
        m.load_state_dict(ck["model_state_dict"], allow_rounded_weights=allow_rounded_weights)
        m.use_official_alignment_heads(name)
        return m

    # ---- stream handling: always run on torch's current stream so torch tensors stay ordered
    def _bind_stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._stream_bound:
            _lib.check(self._lib.wca_engine_set_stream(self._h, C.c_void_p(s)))
            self._stream_bound = s

    def synchronize(self):
        _lib.check(self._lib.wca_engine_synchronize(self._h))

    # ---- hot path entry points (thin wrappers; shapes documented in include/wca.h)
    def log_mel(self, pcm, n_samples=None):
        """pcm: f32 cuda tensor [n] or [B, n] (n <= 480000). Returns [n_mels, 3000] or [B, n_mels, 3000]."""
        single = pcm.dim() == 1
        p = pcm[None] if single else pcm
        p = p.to(self.device, torch.float32).contiguous()
        B, n = p.shape
        if n > N_SAMPLES:
            p = p[:, :N_SAMPLES].contiguous()
            n = N_SAMPLES
        ns = [n] * B if n_samples is None else [min(int(v), n) for v in n_samples]
        out = torch.empty(B, self.dims.n_mels, N_FRAMES, device=self.device, dtype=torch.float32)
        self._bind_stream()
        for b0 in range(0, B, self.max_batch):
            b1 = min(B, b0 + self.max_batch)
            _lib.check(self._lib.wca_log_mel(self._h, _ptr(p[b0:b1]), n, _lib.i32_array(ns[b0:b1]), b1 - b0, _ptr(out[b0:b1])))
        return out[0] if single else out

    def log_mel_long(self, pcm):
        """whisper.log_mel_spectrogram(pcm, n_mels, padding=N_SAMPLES) of a whole recording (C ABI wca_log_mel_long): pcm f32 [n],
        any n -> [n_mels, (n + 480000) // 160] f32 on the GPU, one `max - 8` floor over the whole recording. The tensor is the
        caller's: the engine keeps no buffer of the recording's size."""
        if pcm.dim() != 1:
            raise ValueError("log_mel_long takes one recording [n]; got shape %s" % (tuple(pcm.shape),))
        p = pcm.to(self.device, torch.float32).contiguous()
        n = p.shape[0]
        T = (n + N_SAMPLES) // 160
        out = torch.empty(self.dims.n_mels, T, device=self.device, dtype=torch.float32)
        self._bind_stream()
        _lib.check(self._lib.wca_log_mel_long(self._h, _ptr(p) if n else None, n, _ptr(out), T, None))
        return out

    def resample(self, pcm, sr_in):
        """whisper.load_audio's resampling step on the GPU (C ABI wca_resample_16k): pcm f32 [n] or [C, n] (C <= 8 channels, averaged)
        sampled at sr_in Hz, on the host or on the device -> cuda f32 [ceil(n * 16000 / sr_in)] at 16 kHz. The filter is
        torchaudio.functional.resample's default (include/wca.h); sr_in == 16000 copies (the channel mean). The tensor is the caller's."""
        if pcm.dim() not in (1, 2):
            raise ValueError("resample takes one recording [n] or [channels, n]; got shape %s" % (tuple(pcm.shape),))
        p = pcm.to(self.device, torch.float32)
        p = p[None] if p.dim() == 1 else p
        if p.stride(1) != 1 and p.shape[1] > 1:
            p = p.contiguous()
        channels, n = p.shape
        ld = p.stride(0) if channels > 1 else n
        L, M = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.wca_resample_plan(int(sr_in), C.byref(L), C.byref(M), None, None))
        out = torch.empty(-(-n * L.value // M.value), device=self.device, dtype=torch.float32)
        n_out = C.c_int64(0)
        self._bind_stream()
        _lib.check(self._lib.wca_resample_16k(self._h, _ptr(p) if n else None, channels, ld, n, int(sr_in), _ptr(out) if n else None,
                                              out.shape[0], C.byref(n_out)))
        assert n_out.value == out.shape[0]
        return out

    def mel_window(self, mel_long, seek, size):
        """pad_or_trim(mel_long[:, seek : seek + size], 3000) (C ABI wca_mel_window). mel_long [n_mels, T] f32 cuda; seek / size ints ->
        [n_mels, 3000], or equally long lists -> [B, n_mels, 3000]; exact zeros beyond `size`."""
        single = not isinstance(seek, (list, tuple))
        seeks, sizes = ([seek], [size]) if single else (list(seek), list(size))
        if len(seeks) != len(sizes):
            raise ValueError("seek and size must have the same length")
        if any(not -2 ** 31 <= int(v) < 2 ** 31 for v in seeks + sizes):
            raise ValueError("seek / size do not fit the C ABI's int32")
        if mel_long.dim() != 2 or mel_long.shape[0] != self.dims.n_mels or mel_long.dtype != torch.float32 or mel_long.stride(1) != 1:
            raise ValueError("mel_long must be an f32 [n_mels, T] tensor with unit frame stride")
        mel_long = mel_long.to(self.device)
        out = torch.empty(len(seeks), self.dims.n_mels, N_FRAMES, device=self.device, dtype=torch.float32)
        self._bind_stream()
        for b0 in range(0, len(seeks), self.max_batch):
            b1 = min(len(seeks), b0 + self.max_batch)
            _lib.check(self._lib.wca_mel_window(self._h, _ptr(mel_long), mel_long.stride(0), mel_long.shape[1], _lib.i32_array(seeks[b0:b1]),
                                                _lib.i32_array(sizes[b0:b1]), b1 - b0, _ptr(out[b0:b1])))
        return out[0] if single else out

    def quiet_cuts(self, mel_long, n_pieces, radius=500, half_width=12, content_frames=None):
        """Where to cut a long recording into n_pieces pieces (C ABI wca_quiet_cuts: near each equal share, the even frame with the lowest
        level smoothed over 2 half_width + 1 frames, within `radius` frames). mel_long [n_mels, T] f32 cuda as log_mel_long leaves it;
        content_frames defaults to T - 3000, the recording without its 30 s of padding. Returns (cuts: n_pieces + 1 frames from 0 to
        content_frames, strictly increasing; levels: the n_pieces - 1 smoothed levels at the interior cuts) as lists of ints."""
        if mel_long.dim() != 2 or mel_long.shape[0] != self.dims.n_mels or mel_long.dtype != torch.float32 or mel_long.stride(1) != 1:
            raise ValueError("mel_long must be an f32 [n_mels, T] tensor with unit frame stride")
        mel_long = mel_long.to(self.device)
        if content_frames is None:
            content_frames = mel_long.shape[1] - N_FRAMES
        if int(content_frames) > mel_long.shape[1]:
            raise ValueError("content_frames %d beyond the %d frames of mel_long" % (content_frames, mel_long.shape[1]))
        n = int(n_pieces)
        cuts = np.zeros(max(n, 1) + 1, dtype=np.int32)
        levels = np.zeros(max(n - 1, 1), dtype=np.int32)
        self._bind_stream()
        _lib.check(self._lib.wca_quiet_cuts(self._h, _ptr(mel_long), mel_long.stride(0), int(content_frames), n, int(radius), int(half_width),
                                            cuts.ctypes.data_as(_lib._pi32), levels.ctypes.data_as(_lib._pi32)))
        return [int(v) for v in cuts], [int(v) for v in levels[:n - 1]]

    def speech_segments(self, mel_long, content_frames=None, **vad_options):
        """Speech activity of a long recording (C ABI wca_speech_segments; include/wca.h has the exact definition): the frame ranges whose
        smoothed log-mel level stands out of the recording's own noise floor, after hysteresis, closing of short gaps, removal of short
        runs and padding. mel_long [n_mels, T] f32 cuda as log_mel_long leaves it; content_frames defaults to T - 3000. vad_options:
        half_width, floor_permille, peak_permille, on_share, off_share, min_range, min_speech, min_silence, pad (_lib.VAD_DEFAULTS; the
        durations in frames of 10 ms). Returns (segments: list of (start, stop) frames, in order, never truncated; stats: {"lo", "hi",
        "on_thr", "off_thr", "flat", "n_segments"}). A recording whose level range is below min_range is "flat": one segment (0,
        content_frames). The kernels are exact against the definition; the defaults' quality on real speech is not established."""
        unknown = set(vad_options) - set(_lib.VAD_DEFAULTS)
        if unknown:
            raise ValueError("unknown VAD option(s) %s; the options are %s" % (sorted(unknown), list(_lib.VAD_DEFAULTS)))
        if mel_long.dim() != 2 or mel_long.shape[0] != self.dims.n_mels or mel_long.dtype != torch.float32 or mel_long.stride(1) != 1:
            raise ValueError("mel_long must be an f32 [n_mels, T] tensor with unit frame stride")
        mel_long = mel_long.to(self.device)
        if content_frames is None:
            content_frames = mel_long.shape[1] - N_FRAMES
        content_frames = int(content_frames)
        if content_frames > mel_long.shape[1]:
            raise ValueError("content_frames %d beyond the %d frames of mel_long" % (content_frames, mel_long.shape[1]))
        opts = _lib.VadOpts(**{k: int(v) for k, v in dict(_lib.VAD_DEFAULTS, **vad_options).items()})
        cap = (max(content_frames, 0) + 1) // 2   # more runs than that do not fit
        pairs = np.zeros((max(cap, 1), 2), dtype=np.int32)
        stats = np.zeros(6, dtype=np.int32)
        self._bind_stream()
        _lib.check(self._lib.wca_speech_segments(self._h, _ptr(mel_long), mel_long.stride(0), content_frames, C.byref(opts),
                                                 pairs.ctypes.data_as(_lib._pi32), cap, stats.ctypes.data_as(_lib._pi32)))
        names = ("lo", "hi", "on_thr", "off_thr", "flat", "n_segments")
        return [(int(a), int(b)) for a, b in pairs[:int(stats[5])]], {k: int(v) for k, v in zip(names, stats)}

    def transcribe(self, audio, **kw):
        """whisper.transcribe(model, audio, ...) at temperature 0 with this project's word aligner (transcribe.transcribe)."""
        from . import transcribe as _t
        return _t.transcribe(self, audio, **kw)

    def force_align_long(self, audio, text, **kw):
        """Word times of a recording of any length against its given transcript (align_long.force_align_long)."""
        from . import align_long as _a
        return _a.force_align_long(self, audio, text, **kw)

    def force_align_cues(self, audio, cues, **kw):
        """Word times of a recording against its subtitle cues, a list of (start_s, end_s, text) or an .srt / .vtt path
        (align_long.force_align_cues)."""
        from . import align_long as _a
        return _a.force_align_cues(self, audio, cues, **kw)

    def force_align_cues_batch(self, audios, cues, **kw):
        """force_align_cues() of several recordings, their windows sharing the rounds (align_long.force_align_cues_batch)."""
        from . import align_long as _a
        return _a.force_align_cues_batch(self, audios, cues, **kw)

    def force_align_long_batch(self, audios, texts, **kw):
        """force_align_long() of several recordings in lock-step, one align_batch per round (align_long.force_align_long_batch)."""
        from . import align_long as _a
        return _a.force_align_long_batch(self, audios, texts, **kw)

    def transcribe_batch(self, audios, **kw):
        """transcribe() of several recordings in lock-step, one decode batch per round (transcribe.transcribe_batch)."""
        from . import transcribe as _t
        return _t.transcribe_batch(self, audios, **kw)

    def get_attentions(self, mel, tokens, max_frames, medfilt_width=7, qk_scale=1.0, n_tok=None, want_logits=True):
        """mel [B,n_mels,3000] f32, tokens [B,n] int64, max_frames list[int] -> (weights [B,L,H,n,F], logits [B,n,V])."""
        mel = mel.to(self.device, torch.float32).contiguous()
        tokens = tokens.to(self.device, torch.int64).contiguous()
        B, n = tokens.shape
        if B > self.max_batch:
            raise ValueError("batch %d > engine max_batch %d" % (B, self.max_batch))
        mf = [int(v) for v in max_frames]
        F = max(mf)
        L, H = self.dims.n_text_layer, self.dims.n_text_head
        weights = torch.empty(B, L, H, n, max(F, 1), device=self.device, dtype=torch.float32)
        logits = torch.empty(B, n, self.dims.n_vocab, device=self.device, dtype=torch.float32) if want_logits else None
        self._bind_stream()
        nt = _lib.i32_array(n_tok) if n_tok is not None else None
        _lib.check(self._lib.wca_get_attentions(self._h, _ptr(mel), _ptr(tokens), B, n, nt, _lib.i32_array(mf),
                                                int(medfilt_width), float(qk_scale), _ptr(weights), _ptr(logits)))
        return weights, logits

    def encode(self, mel):
        """Encoder only (tests): mel [B,n_mels,3000] -> ln_post output [B,1500,d] f32."""
        mel = mel.to(self.device, torch.float32).contiguous()
        B = mel.shape[0]
        out = torch.empty(B, 1500, self.dims.n_audio_state, device=self.device, dtype=torch.float32)
        self._bind_stream()
        _lib.check(self._lib.wca_test_encoder(self._h, _ptr(mel), B, _ptr(out)))
        return out

    def make_opts(self, aggregation="mean", topk=-1, w_colnorm=1.0, w_rownorm=1.0, w_coverage=0.0, sot_len=3,
                  medfilt_width=7, qk_scale=1.0):
        if aggregation not in ("mean", "topk"):
            raise ValueError("aggregation must be 'mean' or 'topk'")
        if aggregation == "topk":
            assert topk > 0  # timing.py:92
        return _lib.AlignOpts(_lib.AGGR_TOPK if aggregation == "topk" else _lib.AGGR_MEAN, int(topk), float(w_colnorm),
                              float(w_rownorm), float(w_coverage), int(sot_len), int(medfilt_width), float(qk_scale))

    def align_batch(self, pcm, n_samples, tokens, n_tok, max_frames, opts, enqueue_only=False, token_logprobs_vocab_end=None, open_end=None,
                    path_scores=False, row_windows=None, alignment_heads=None):
        """Fused pipeline. pcm [B,stride] f32 cuda, tokens [B,n_max] int64 cuda. Returns (jump_frames [B,n_max] int32, sel [B,topk]).
        token_logprobs_vocab_end (tokenizer.eot): the teacher tokens' log-probabilities are computed on the GPU as well
        (wca_align_desc.vocab_end) and returned as a third value [B,n_max] f32 (row b: n_tok[b] - sot_len - 2 entries, then 0);
        after enqueue_only=True, fetch them with fetch(..., with_token_logprobs=True).
        open_end (B bools): row b's DTW is open-ended where open_end[b] (wca_align_desc.open_end_host: the path ends in the last frame at
        the text row that fits best; a row with False gets exactly the closed result). The end rows [B] int32 and the scores [B] f32 are
        returned as two further values, after the log-probs where those are asked for; rows past a row's end row have jump frame -1.
        After enqueue_only=True, fetch them with fetch(..., with_end_rows=True). None: nothing changes.
        path_scores: the path-score kernel runs behind the DTW (wca_align_desc.path_scores) and (path_mean [B,n_max] f32, path_cells
        [B,n_max] int32) are the LAST two values returned: per DTW row, laid out like the jump frames, the mean of the aggregated matrix
        over the path's cells in that row and their number. After enqueue_only=True, fetch them with fetch(..., with_path_scores=True).
        row_windows = (lo, hi), each [B, n_max] int32 (or nested lists of that shape): DTW row i of batch row b may only sit at the encoder
        frames lo[b][i] <= j <= hi[b][i] (wca_align_batch_enqueue_windows; DTW rows count from the first token after the sot sequence and
        no_timestamps, the eot is the last, later entries are not read). The windows must be valid (include/wca.h wca_dtw_windows), and an
        open_end row takes full windows only; otherwise the engine refuses the call (WcaError) before anything is enqueued. The returned
        values are those without windows. None: nothing changes and no new code runs.
        alignment_heads: a list of (layer, head) pairs, or True for self.alignment_heads: the batch takes the ALIGNMENT-HEADS route
        (wca_align_batch_enqueue_heads): openai-whisper's own post-processing of those heads -- softmax, (w - mean) / std per frame over the
        tokens, median filter, mean over the heads in the order given -- in place of head scoring, top-k and aggregation; of opts only
        sot_len, medfilt_width and qk_scale are read. The return shape is unchanged (sel is None). Not together with path_scores,
        open_end or row_windows (ValueError). After enqueue_only=True the batch holds no top-k slot whatever opts says: fetch it with
        fetch(B, n_max, None, ...) (opts=None: no selected heads), not with top-k opts. None: nothing changes and no new code runs."""
        B, n_max = tokens.shape
        heads = None
        if alignment_heads is not None and alignment_heads is not False:
            if path_scores or open_end is not None or row_windows is not None:
                raise ValueError("alignment_heads cannot be combined with path_scores, open_end or row_windows: the path score is defined on "
                                 "the [0, 1] aggregation, and the alignment-heads matrix has no open-ended or windowed DTW")
            heads = self.flat_heads(self.alignment_heads if alignment_heads is True else alignment_heads)
        if open_end is not None and len(open_end) != B:
            raise ValueError("open_end lists %d flags for %d rows" % (len(open_end), B))
        self._bind_stream()
        # pcm=None re-uses the encoder state left by the preceding greedy_decode of the same batch
        ns = _lib.i32_array(n_samples) if n_samples is not None else None
        nt, mf = _lib.i32_array(n_tok), _lib.i32_array(max_frames)
        oe = _lib.i32_array([bool(v) for v in open_end]) if open_end is not None else None
        d = _lib.AlignDesc(pcm_dev=_ptr(pcm), n_samples_host=_ptr(ns), tokens_dev=_ptr(tokens), n_tok_host=_ptr(nt), max_frames_host=_ptr(mf),
                           opts=C.pointer(opts), open_end_host=_ptr(oe), pcm_stride=pcm.shape[1] if pcm is not None else 0, n_tok_max=n_max,
                           batch=B, vocab_end=int(token_logprobs_vocab_end or 0), path_scores=1 if path_scores else 0)
        if heads is not None:
            _lib.check(self._lib.wca_align_batch_enqueue_heads(self._h, C.byref(d), heads.ctypes.data_as(_pi32), len(heads)))
            opts = None   # (what fetch reads of it: no top-k slot)
        elif row_windows is not None:
            lo, hi = (np.ascontiguousarray(w, dtype=np.int32) for w in row_windows)
            if lo.shape != (B, n_max) or hi.shape != (B, n_max):
                raise ValueError("row_windows are two [%d, %d] tables, got %s and %s" % (B, n_max, lo.shape, hi.shape))
            _lib.check(self._lib.wca_align_batch_enqueue_windows(self._h, C.byref(d), lo.ctypes.data_as(_pi32), hi.ctypes.data_as(_pi32)))
        else:
            _lib.check(self._lib.wca_align_batch_enqueue(self._h, C.byref(d)))
        if enqueue_only:
            return None
        return self.fetch(B, n_max, opts, with_token_logprobs=token_logprobs_vocab_end is not None, with_end_rows=open_end is not None,
                          with_path_scores=bool(path_scores))

    def flat_heads(self, heads):
        """(layer, head) pairs -> the int32 array layer * n_text_head + head the C ABI takes, in the order given; ValueError for an empty
        list or a pair outside the model."""
        pairs = [(int(l), int(h)) for l, h in heads]
        if not pairs:
            raise ValueError("alignment_heads is empty")
        for l, h in pairs:
            if not (0 <= l < self.dims.n_text_layer and 0 <= h < self.dims.n_text_head):
                raise ValueError("alignment head (%d, %d) out of range" % (l, h))
        return np.ascontiguousarray([l * self.dims.n_text_head + h for l, h in pairs], dtype=np.int32)

    def encode_batch(self, mel=None, pcm=None, n_samples=None):
        """C ABI wca_encode_batch: enqueue log-mel/encoder/cross-K/V of a micro-batch (no host sync). The state is picked up
        by greedy_decode(None, None, None, ..., batch=B) and by align_batch(pcm=None, ...)."""
        self._bind_stream()
        B = mel.shape[0] if mel is not None else pcm.shape[0]
        if mel is not None:
            mel = mel.contiguous().float()
        _lib.check(self._lib.wca_encode_batch(self._h, _ptr(mel) if mel is not None else None, _ptr(pcm) if pcm is not None else None,
                                              pcm.shape[1] if pcm is not None else 0,
                                              _lib.i32_array(n_samples) if n_samples is not None else None, B))
        if not hasattr(self, "_keep"):
            import collections
            self._keep = collections.deque(maxlen=3)
        self._keep.append((mel, pcm))  # the kernels read these buffers asynchronously; up to two encodes are in flight
        return B

    def _decode(self, mel, pcm, n_samples, batch, init, n_init, sot_index, sample_len, opts, suppress_mask, blank_mask, per_row, prefill,
                temps=None, seeds=None, redecode=False, group=None):
        """What the four decode methods share: the masks, the output arrays, the wca_decode_desc around the caller's row arrays (init [n] or
        [B, n_max], n_init / sot_index / sample_len: one int or one per row), the call, and last_no_speech_prob. group = (n_group, mode,
        max_candidates, n_slot): wca_decode_group, whose outputs hold n_slot sequences per audio and the [B] counts n_out behind them.
        Every array a descriptor points to is a local of this frame until the call has returned."""
        self._bind_stream()
        B = _batch_size(mel, pcm, batch)
        T = max((int(n) + int(sl) for n, sl in zip(n_init, sample_len)), default=1)
        slots = (B,) if group is None else (B, group[3])
        tokens = np.zeros(slots + (max(T, 1),), dtype=np.int32)
        n_tok = np.zeros(slots, dtype=np.int32)
        lp = np.zeros(slots, dtype=np.float32)
        sup = np.ascontiguousarray(suppress_mask, dtype=np.uint8)
        blank = np.ascontiguousarray(blank_mask, dtype=np.uint8) if blank_mask is not None else None
        if sup.shape[0] != self.dims.n_vocab or (blank is not None and blank.shape[0] != self.dims.n_vocab):
            raise ValueError("filter masks must have n_vocab entries")
        nsp = np.full(B, np.nan, dtype=np.float32)
        if mel is not None:
            mel = mel.contiguous().float()
        ns = _lib.i32_array(n_samples) if n_samples is not None else None
        ni, si, sl = _lib.i32_array(n_init), _lib.i32_array(sot_index), _lib.i32_array(sample_len)
        out = dict(tokens_out_host=_ptr(tokens), n_tokens_host=_ptr(n_tok), sum_logprob_host=_ptr(lp),
                   no_speech_prob_host=_ptr(nsp if opts.no_speech >= 0 else None))   # the group descriptor's where there is one
        d = _lib.DecodeDesc(mel_dev=_ptr(mel), pcm_dev=_ptr(pcm), n_samples_host=_ptr(ns), initial_tokens_host=_ptr(init), n_initial_host=_ptr(ni),
                            sot_index_host=_ptr(si), sample_len_host=_ptr(sl), temperature_host=_ptr(temps), seed_host=_ptr(seeds),
                            suppress_mask_host=_ptr(sup), blank_mask_host=_ptr(blank), opts=C.pointer(opts),
                            pcm_stride=pcm.shape[1] if pcm is not None else 0, batch=B, per_row=per_row, prefill=int(prefill),
                            redecode=1 if redecode else 0, **({} if group else out))
        if group is None:
            _lib.check(self._lib.wca_decode(self._h, C.byref(d)))
            self.last_no_speech_prob = nsp
            return tokens, n_tok, lp
        n_out = np.zeros(B, dtype=np.int32)
        g = _lib.GroupDesc(n_out_host=_ptr(n_out), n_group=group[0], mode=group[1], max_candidates=group[2], **out)
        _lib.check(self._lib.wca_decode_group(self._h, C.byref(d), C.byref(g)))
        self.last_no_speech_prob = nsp
        return tokens, n_tok, lp, n_out

    def greedy_decode(self, mel, pcm, n_samples, initial_tokens, suppress_mask, blank_mask, sample_len, eot, timestamp_begin,
                      apply_timestamp_rules=True, max_initial_timestamp_index=50, batch=None, no_speech=-1, sot_index=0, prefill=0):
        """C ABI wca_decode with one row description for every row. mel [B,n_mels,3000] f32 cuda XOR pcm [B,stride] f32 cuda (+ n_samples).
        Returns (tokens [B, n_initial+sample_len] int32, n_tokens [B] int32, sum_logprobs [B] f32) as numpy arrays; the
        encoder state stays in the engine for a following align_batch(pcm=None, ...). With no_speech >= 0 (the
        <|nospeech|> token id) self.last_no_speech_prob [B] holds DecodingResult.no_speech_prob.
        sot_index: position of <|sot|> in initial_tokens (no_speech_prob is read there); prefill=1: one batched forward
        over the initial tokens instead of one decode step per position. n_initial + sample_len may reach n_text_ctx + 1."""
        opts = _lib.DecodeOpts(int(sample_len), int(eot), int(timestamp_begin), 1 if apply_timestamp_rules else 0, int(max_initial_timestamp_index),
                               int(no_speech))
        return self._decode(mel, pcm, n_samples, batch, _lib.i32_array(initial_tokens), [len(initial_tokens)], [sot_index], [sample_len], opts,
                            suppress_mask, blank_mask, 0, prefill)

    def greedy_decode_rows(self, mel, pcm, n_samples, initial_tokens, sot_index, sample_len, suppress_mask, blank_mask, eot, timestamp_begin,
                           apply_timestamp_rules=True, max_initial_timestamp_index=50, batch=None, no_speech=-1):
        """C ABI wca_decode with per_row = 1: greedy_decode with initial tokens, <|sot|> position and sample budget PER ROW (initial_tokens: one
        token list per row, of any lengths; sot_index, sample_len: one int per row). Returns (tokens [B, T_max] int32 with
        T_max = max_b(len(initial_tokens[b]) + sample_len[b]), row b left-aligned; n_tokens [B]: row b's sampled tokens are
        tokens[b, len(initial_tokens[b]) : n_tokens[b]]; sum_logprobs [B]); self.last_no_speech_prob as greedy_decode. The initial
        tokens always go through the batched prefill; the encoder state stays for a following align_batch(pcm=None, ...)."""
        return self._decode_rows(mel, pcm, n_samples, initial_tokens, sot_index, sample_len, suppress_mask, blank_mask, eot, timestamp_begin,
                                 apply_timestamp_rules, max_initial_timestamp_index, batch, no_speech)

    def decode_rows_sampled(self, mel, pcm, n_samples, initial_tokens, sot_index, sample_len, suppress_mask, blank_mask, eot, timestamp_begin,
                            apply_timestamp_rules=True, max_initial_timestamp_index=50, batch=None, no_speech=-1, temperature=None, seed=None,
                            redecode=False):
        """greedy_decode_rows with a temperature (float >= 0) and a seed (int, taken mod 2^64) PER ROW (wca_decode_desc.temperature_host /
        seed_host). A row at temperature 0 is decoded greedily, bit for bit as greedy_decode_rows decodes it; a row at T > 0 draws each token from
        softmax(filtered logits / T) by Gumbel-max with Philox noise keyed by its seed and counted by its sampled tokens, so a row's draws
        do not depend on where in the batch it sits. sum_logprobs accumulates the untempered log-probability, as upstream does.
        redecode=True (mel = pcm = None, batch=B): decode again the state the previous decode of these B rows left for
        align_batch(pcm=None), with no encoder pass; the state is still there for the alignment afterwards."""
        temps, seeds = _temps_seeds(_batch_size(mel, pcm, batch), temperature, seed)
        return self._decode_rows(mel, pcm, n_samples, initial_tokens, sot_index, sample_len, suppress_mask, blank_mask, eot, timestamp_begin,
                                 apply_timestamp_rules, max_initial_timestamp_index, batch, no_speech, temps, seeds, redecode)

    def _decode_rows(self, mel, pcm, n_samples, initial_tokens, sot_index, sample_len, suppress_mask, blank_mask, eot, timestamp_begin,
                     apply_timestamp_rules, max_initial_timestamp_index, batch, no_speech, temps=None, seeds=None, redecode=False, group=None):
        """The per-row arrays that greedy_decode_rows, decode_rows_sampled and decode_group pass."""
        B = _batch_size(mel, pcm, batch)
        rows = [[int(t) for t in r] for r in initial_tokens]
        if not (len(rows) == len(sot_index) == len(sample_len) == B):
            raise ValueError("initial_tokens, sot_index and sample_len take one entry per batch row (%d)" % B)
        n_init = [len(r) for r in rows]
        n_max = max(n_init) if n_init else 0
        init = np.full((B, max(n_max, 1)), int(eot), dtype=np.int32)
        for b, r in enumerate(rows):
            init[b, :len(r)] = r
        opts = _lib.DecodeOpts(max(int(v) for v in sample_len) if B else 0, int(eot), int(timestamp_begin), 1 if apply_timestamp_rules else 0,
                               int(max_initial_timestamp_index), int(no_speech))
        return self._decode(mel, pcm, n_samples, batch, init, n_init, sot_index, sample_len, opts, suppress_mask, blank_mask, 1, 1, temps, seeds,
                            redecode, group)

    def decode_group(self, mel, pcm, n_samples, initial_tokens, sot_index, sample_len, suppress_mask, blank_mask, eot, timestamp_begin,
                     apply_timestamp_rules=True, max_initial_timestamp_index=50, batch=None, no_speech=-1, n_group=1, mode=0, max_candidates=None,
                     temperature=None, seed=None, redecode=False):
        """C ABI wca_decode_group: greedy_decode_rows' per-row arrays for the B audios, n_group decoder rows per audio that share its
        cross-K/V. mode 0: beam search with beam_size = n_group and max_candidates = round(beam_size * patience) (default n_group); mode 1:
        n_group independent samples per audio at temperature[b], sample g drawing with decoding.group_seed(seed[b], g).
        Returns (tokens [B, n_slot, T_max] int32, n_tokens [B, n_slot] int32, sum_logprobs [B, n_slot] f32, n_out [B] int32) with
        n_slot = max(n_group, max_candidates) for the beam and n_group for samples: the first n_out[b] slots of audio b hold a sequence
        (beam: the finished list in the order it filled, then the live beams that top it up; samples: sample g in slot g), whose sampled
        tokens are tokens[b, i, len(initial_tokens[b]) : n_tokens[b, i]]. The ranking is the caller's (decoding.rank_sequences).
        self.last_no_speech_prob [B] as greedy_decode; the encoder state stays for a following align_batch(pcm=None, ...)."""
        G, mode = int(n_group), int(mode)
        if mode not in (0, 1):
            raise ValueError("mode is 0 (beam) or 1 (independent samples)")
        max_candidates = G if max_candidates is None else int(max_candidates)
        n_slot = max(G, max_candidates) if mode == 0 else G
        if G < 1 or n_slot < 1:
            raise ValueError("n_group and max_candidates must be at least 1")
        temps = seeds = None
        if temperature is not None or seed is not None:
            temps, seeds = _temps_seeds(_batch_size(mel, pcm, batch), temperature, seed)
        return self._decode_rows(mel, pcm, n_samples, initial_tokens, sot_index, sample_len, suppress_mask, blank_mask, eot, timestamp_begin,
                                 apply_timestamp_rules, max_initial_timestamp_index, batch, no_speech, temps, seeds, redecode,
                                 (G, mode, max_candidates, n_slot))

    def beam_trace(self):
        """Test accessor (C ABI wca_test_beam_trace): what the last beam search chose -> [steps, rows, 2] int32, entry (c, r) = (the row
        whose beam row r continues after choice c, the token it appended; -1 for a row past its budget)."""
        steps, rows = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.wca_test_beam_trace(self._h, C.byref(steps), C.byref(rows), None, 0))
        trace = np.zeros((max(steps.value, 1), max(rows.value, 1), 2), dtype=np.int32)
        _lib.check(self._lib.wca_test_beam_trace(self._h, C.byref(steps), C.byref(rows), trace.ctypes.data_as(_lib._pi32), trace.size))
        return trace[:steps.value, :rows.value]

    def detect_language(self, mel=None, tokenizer=None, *, pcm=None, n_samples=None, batch=None, sot=None, lang_begin=None, n_lang=None):
        """model.detect_language(mel, tokenizer) -> (language_tokens, language_probs), upstream's schema (decoding.detect_language).
        With sot / lang_begin / n_lang it is the thin C ABI call (wca_detect_language): mel [B,n_mels,3000] f32 cuda XOR pcm [B,stride]
        f32 cuda (+ n_samples), or neither with batch=B (the state queued by encode_batch) -> (lang_token [B] int32, probs [B, n_lang] f32)
        as numpy arrays. The encoded state stays in the engine for a following decode(..., encoded_batch=B)."""
        if sot is None:
            from . import decoding
            return decoding.detect_language(self, mel, tokenizer, pcm=pcm, n_samples=n_samples)
        self._bind_stream()
        B = _batch_size(mel, pcm, batch)
        if mel is not None:
            mel = mel.to(self.device).contiguous().float()
        lang = np.zeros(max(B, 1), dtype=np.int32)
        probs = np.zeros((max(B, 1), max(int(n_lang), 1)), dtype=np.float32)
        _lib.check(self._lib.wca_detect_language(
            self._h, _ptr(mel) if mel is not None else None, _ptr(pcm) if pcm is not None else None, pcm.shape[1] if pcm is not None else 0,
            _lib.i32_array(n_samples) if n_samples is not None else None, B, int(sot), int(lang_begin), int(n_lang),
            lang.ctypes.data_as(_lib._pi32), probs.ctypes.data_as(_lib._pf)))
        return lang[:B], probs[:B]

    def last_decode_positions(self):
        """(positions per row fed by the batched prefill, positions fed one decode step at a time) of the last greedy_decode."""
        pre, step = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.wca_last_decode_positions(self._h, C.byref(pre), C.byref(step)))
        return pre.value, step.value

    def decode_state(self, batch, T_max, logits_rows=None):
        """Test accessor (C ABI wca_test_decode_state): what the last decode (greedy_decode, greedy_decode_rows, decode_rows_sampled or
        decode_group) left on the device -> (logits [logits_rows, n_vocab] f32, cache [n_text_layer, 2, batch, T_max, n_text_state] f16) as
        numpy arrays. T_max is that call's largest n_initial + sample_len; logits_rows defaults to batch (2 * batch: with the <|sot|> rows of
        a prefill with no_speech). After decode_group batch is its B * n_group decoder rows, row b * n_group + g = beam or sample g of audio
        b: the cache is the half of the two that the last reorder wrote (beam: the rows of the beams after the last choice, slots
        [0, n_initial + choices - 1); samples: each row's own), the logits are the last step's B * n_group rows (beam: the beams before the
        last choice), and the rows of an audio past its budget hold, past what they had fed at their last choice, what is never read."""
        rows = int(batch if logits_rows is None else logits_rows)
        logits = np.zeros((max(rows, 1), self.dims.n_vocab), dtype=np.float32)
        cache = np.zeros((self.dims.n_text_layer, 2, max(int(batch), 1), max(int(T_max), 1), self.dims.n_text_state), dtype=np.float16)
        _lib.check(self._lib.wca_test_decode_state(self._h, int(batch), int(T_max), rows, logits.ctypes.data_as(_lib._pf),
                                                   cache.ctypes.data_as(C.c_void_p)))
        return logits, cache

    def decode(self, mel, options=None):
        """whisper.decode(model, mel, options) (infer_ali.py:60)."""
        from . import decoding
        return decoding.decode(self, mel, options if options is not None else decoding.DecodingOptions())

    def align_postproc(self, qk, n_tok, n_frames, opts, L, H, n_frames_max=None, open_end=None, path_scores=False):
        """C ABI wca_test_align_postproc (tests): phase 2's post-processing of align_batch on given logits qk [B, L*H, n_tok_max, ld] f32
        cuda. Returns a dict of numpy arrays: scores [B,LH], colnorm [B,LH,F], rowstats [B,LH,n_tok_max,2], sel [B,topk] (None for
        'mean'), matrix [B,n_tok_max,F], jump [B,n_tok_max]; F = n_frames_max (default: the largest n_frames). Only utterance b's own
        corner of an array is defined. path_scores: through wca_test_align_postproc_scores, which adds path_mean [B,n_tok_max] f32 and
        path_cells [B,n_tok_max] int32."""
        qk = qk.to(self.device, torch.float32).contiguous()
        B, LH, n_max, ld = qk.shape
        if LH != L * H:
            raise ValueError("qk holds %d heads, not %d x %d" % (LH, L, H))
        F = int(n_frames_max) if n_frames_max is not None else max(int(v) for v in n_frames)
        k = opts.topk if opts.aggregation == _lib.AGGR_TOPK else 0
        out = {"scores": np.zeros((B, LH), np.float32), "colnorm": np.zeros((B, LH, max(F, 1)), np.float32),
               "rowstats": np.zeros((B, LH, n_max, 2), np.float32), "sel": np.zeros((B, k), np.int32) if k > 0 else None,
               "matrix": np.zeros((B, n_max, max(F, 1)), np.float32), "jump": np.zeros((B, n_max), np.int32)}
        nt, nf = _lib.i32_array(n_tok), _lib.i32_array(n_frames)
        oe = _lib.i32_array([bool(v) for v in open_end]) if open_end is not None else None
        self._bind_stream()
        d = _lib.PostprocDesc(qk_dev=_ptr(qk), n_tok_host=_ptr(nt), n_frames_host=_ptr(nf), open_end_host=_ptr(oe), opts=C.pointer(opts),
                              scores_host=_ptr(out["scores"]), colnorm_host=_ptr(out["colnorm"]), rowstats_host=_ptr(out["rowstats"]),
                              sel_idx_host=_ptr(out["sel"]), matrix_host=_ptr(out["matrix"]), jump_host=_ptr(out["jump"]),
                              B=B, L=L, H=H, n_tok_max=n_max, ld=ld, n_frames_max=F)
        if path_scores:
            out["path_mean"], out["path_cells"] = np.zeros((B, n_max), np.float32), np.zeros((B, n_max), np.int32)
            _lib.check(self._lib.wca_test_align_postproc_scores(self._h, C.byref(d), out["path_mean"].ctypes.data_as(_pf32),
                                                                out["path_cells"].ctypes.data_as(_pi32)))
        else:
            _lib.check(self._lib.wca_test_align_postproc(self._h, C.byref(d)))
        return out

    def align_heads_postproc(self, qk, n_tok, n_frames, opts, L, H, heads, n_frames_max=None):
        """C ABI wca_test_align_heads_postproc (tests): the alignment-heads post-processing of align_batch(alignment_heads=...) on given
        logits qk [B, L*H, n_tok_max, ld] f32 cuda, over `heads`, flat indices layer * H + head in the order they are summed. Returns a dict
        of numpy arrays: rowstats [B,S,n_tok_max,2] = (max, sum), colstats [B,S,F,2] = (mean, std), matrix [B,n_tok_max,F], jump
        [B,n_tok_max]; F = n_frames_max (default: the largest n_frames). Only utterance b's own corner of an array is defined."""
        qk = qk.to(self.device, torch.float32).contiguous()
        B, LH, n_max, ld = qk.shape
        if LH != L * H:
            raise ValueError("qk holds %d heads, not %d x %d" % (LH, L, H))
        F = int(n_frames_max) if n_frames_max is not None else max(int(v) for v in n_frames)
        hd = np.ascontiguousarray(heads, dtype=np.int32)
        S = len(hd)
        out = {"rowstats": np.zeros((B, max(S, 1), n_max, 2), np.float32), "colstats": np.zeros((B, max(S, 1), max(F, 1), 2), np.float32),
               "matrix": np.zeros((B, n_max, max(F, 1)), np.float32), "jump": np.zeros((B, n_max), np.int32)}
        nt, nf = _lib.i32_array(n_tok), _lib.i32_array(n_frames)
        self._bind_stream()
        d = _lib.HeadsPostprocDesc(qk_dev=_ptr(qk), n_tok_host=_ptr(nt), n_frames_host=_ptr(nf), heads_host=_ptr(hd), opts=C.pointer(opts),
                                   rowstats_host=_ptr(out["rowstats"]), colstats_host=_ptr(out["colstats"]), matrix_host=_ptr(out["matrix"]),
                                   jump_host=_ptr(out["jump"]), B=B, L=L, H=H, n_tok_max=n_max, ld=ld, n_frames_max=F, n_heads=S)
        _lib.check(self._lib.wca_test_align_heads_postproc(self._h, C.byref(d)))
        return out

    def dtw_path_scores(self, matrix_dev, n_rows=None, n_cols=None, open_end=None):
        """C ABI wca_dtw_path_scores: P DTW problems matrix_dev [P, N, M] f32 cuda (NOT negated), problem p the n_rows[p] x n_cols[p] corner
        of its slice (None: all N / all M), open-ended where open_end[p] (None: all closed), each followed by the path-score kernel.
        Returns (jump [P,N] int32, end_rows [P] int32, path_mean [P,N] f32, path_cells [P,N] int32)."""
        m = matrix_dev.to(self.device, torch.float32).contiguous()
        if m.dim() != 3:
            raise ValueError("matrix_dev must be [P, N, M]")
        P, N, M = m.shape
        for name, v in (("n_rows", n_rows), ("n_cols", n_cols), ("open_end", open_end)):
            if v is not None and len(v) != P:
                raise ValueError("%s lists %d values for %d problems" % (name, len(v), P))
        nr = _lib.i32_array(n_rows) if n_rows is not None else None
        nc = _lib.i32_array(n_cols) if n_cols is not None else None
        oe = _lib.i32_array([bool(v) for v in open_end]) if open_end is not None else None
        jump, end_rows = np.zeros((P, N), np.int32), np.zeros(P, np.int32)
        mean, cells = np.zeros((P, N), np.float32), np.zeros((P, N), np.int32)
        self._bind_stream()
        _lib.check(self._lib.wca_dtw_path_scores(self._h, _ptr(m), P, N, M, nr, nc, oe, jump.ctypes.data_as(_pi32), end_rows.ctypes.data_as(_pi32),
                                                 mean.ctypes.data_as(_pf32), cells.ctypes.data_as(_pi32)))
        return jump, end_rows, mean, cells

    def dtw_windows(self, matrix_dev, row_lo, row_hi, n_rows=None, n_cols=None):
        """C ABI wca_dtw_batch_dev_windows: P closed DTW problems matrix_dev [P, N, M] f32 cuda (NOT negated) in which text row i of problem
        p may only sit at the frames row_lo[p][i] <= j <= row_hi[p][i] ([P, N] int32 each); problem p is the n_rows[p] x n_cols[p] corner
        of its slice (None: all N / all M) and only its first n_rows[p] window entries are read. Invalid windows are refused before
        anything runs (include/wca.h wca_dtw_windows). Returns the jump frames [P, N] int32 (0 beyond a problem's rows)."""
        m = matrix_dev.to(self.device, torch.float32).contiguous()
        if m.dim() != 3:
            raise ValueError("matrix_dev must be [P, N, M]")
        P, N, M = m.shape
        lo, hi = np.ascontiguousarray(row_lo, dtype=np.int32), np.ascontiguousarray(row_hi, dtype=np.int32)
        if lo.shape != (P, N) or hi.shape != (P, N):
            raise ValueError("row_lo / row_hi must be [%d, %d], got %s and %s" % (P, N, lo.shape, hi.shape))
        for name, v in (("n_rows", n_rows), ("n_cols", n_cols)):
            if v is not None and len(v) != P:
                raise ValueError("%s lists %d values for %d problems" % (name, len(v), P))
        nr = _lib.i32_array(n_rows) if n_rows is not None else None
        nc = _lib.i32_array(n_cols) if n_cols is not None else None
        jump = np.zeros((P, N), np.int32)
        self._bind_stream()
        _lib.check(self._lib.wca_dtw_batch_dev_windows(self._h, _ptr(m), P, N, M, nr, nc, lo.ctypes.data_as(_pi32), hi.ctypes.data_as(_pi32),
                                                       jump.ctypes.data_as(_pi32)))
        return jump

    def fetch(self, B, n_max, opts, with_token_logprobs=False, with_end_rows=False, with_path_scores=False):
        """Results of the oldest enqueued align_batch: (jump, sel), or (jump, sel, token_logprobs [B,n_max] f32) with
        with_token_logprobs (the batch must have been enqueued with token_logprobs_vocab_end). with_end_rows (the batch must have been
        enqueued with open_end) appends the end rows [B] int32 and the scores [B] f32. with_path_scores (the batch must have been enqueued
        with path_scores) appends, last, path_mean [B,n_max] f32 and path_cells [B,n_max] int32 (wca_align_batch_path_scores).
        opts=None: a batch enqueued with alignment_heads, which selects no heads (sel is None)."""
        k = opts.topk if opts is not None and opts.aggregation == _lib.AGGR_TOPK else 0
        jump = np.zeros((B, n_max), dtype=np.int32)
        sel = np.zeros((B, max(k, 1)), dtype=np.int32)
        lp = np.zeros((B, n_max), dtype=np.float32) if with_token_logprobs else None
        end_rows, scores = (np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.float32)) if with_end_rows else (None, None)
        ps = ()
        if with_path_scores:   # read before the fetch, which consumes the batch
            ps = (np.zeros((B, n_max), dtype=np.float32), np.zeros((B, n_max), dtype=np.int32))
            _lib.check(self._lib.wca_align_batch_path_scores(self._h, B, n_max, ps[0].ctypes.data_as(_pf32), ps[1].ctypes.data_as(_pi32)))
        r = _lib.AlignResult(_ptr(jump), _ptr(sel), _ptr(lp), _ptr(end_rows), _ptr(scores))
        _lib.check(self._lib.wca_align_batch_fetch(self._h, B, n_max, k, C.byref(r)))
        return (jump, (sel if k > 0 else None)) + ((lp,) if with_token_logprobs else ()) + ((end_rows, scores) if with_end_rows else ()) + ps

    def set_profiling(self, on):
        _lib.check(self._lib.wca_set_profiling(self._h, 1 if on else 0))

    def kernel_ms(self, site):
        """(launches, summed ms, algorithmic flops per launch, algorithmic bytes per launch) of one encoder kernel site
        ('qkv' | 'attention' | 'out_proj' | 'fc1' | 'fc2' | 'ln1' | 'ln2') in the last align_batch call (profiling on)."""
        n = C.c_int(0)
        ms = C.c_float(0)
        fl = C.c_double(0)
        by = C.c_double(0)
        _lib.check(self._lib.wca_last_kernel_ms(self._h, _lib.SITES[site], C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
        return n.value, ms.value, fl.value, by.value

    # ---- collation over RCCL through the C ABI (no torch.distributed involved; shard.allgather_results(..., engine=self))
    @staticmethod
    def comm_unique_id():
        """128-byte id of a new communicator (rank 0 creates it; hand it to the other ranks by any side channel)."""
        buf = (C.c_uint8 * 128)()
        _lib.check(_lib.load().wca_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        _lib.check(self._lib.wca_comm_init(self._h, buf, int(rank), int(world)))
        self._comm = (int(rank), int(world))
        return self

    def comm_destroy(self):
        _lib.check(self._lib.wca_comm_destroy(self._h))
        self._comm = None

    @property
    def comm(self):
        """(rank, world) of this engine's RCCL communicator, or None."""
        return getattr(self, "_comm", None)

    def allgather_packed(self, packed):
        """packed: uint8 numpy array of this rank -> list of every rank's uint8 array (wca_allgather_results)."""
        rank, world = self._comm
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        sizes = (C.c_int64 * world)()
        cap = max(int(packed.size), 1 << 16)
        self._bind_stream()
        while True:
            out = np.zeros((world, cap), dtype=np.uint8)
            rc = self._lib.wca_allgather_results(self._h, packed.ctypes.data_as(C.c_void_p), int(packed.size), out.ctypes.data_as(C.c_void_p), cap, sizes)
            if rc == _lib.ERR_TOO_LONG:   # some rank packed more than the smallest `cap` of any rank: EVERY rank gets this verdict
                cap = max(int(v) for v in sizes)   # (decided on the gathered {size, capacity} pairs), and retries with the same room
                continue
            _lib.check(rc)
            return [out[r, :int(sizes[r])].copy() for r in range(world)]

    def allreduce_counters(self, *counters):
        arr = (C.c_int64 * len(counters))(*[int(v) for v in counters])
        self._bind_stream()
        _lib.check(self._lib.wca_allreduce_counters(self._h, arr, len(counters)))
        return tuple(int(v) for v in arr)

    def set_precision(self, mode):
        """'f16': operands rounded to f16 once, fp32 accumulation. 'split' = 'reference' (the contract mode and the engine's
        construction default: what bench.py's `value` and the CLI default use): every operand of every stage as an f16 (hi, lo) pair against
        the exact f16 weights, three-pass attention (wca.h: wca_set_precision) -- the reference's fp32 forward to fp32 summation noise.
        No batch may be in flight; the activation arena is re-created when the engine leaves or enters f16."""
        modes = {"f16": 0, "split": 1, "reference": 1}
        if mode not in modes:
            raise ValueError("precision must be 'f16', 'reference' or 'split'")
        _lib.check(self._lib.wca_set_precision(self._h, modes[mode]))
        return self

    @property
    def precision_sites(self):
        """(stages on (hi, lo) operand pairs, first encoder block): every stage in split mode, none in f16."""
        return (list(_lib.PRECISION_SITES) if self.precision == "split" else []), 0

    @property
    def precision(self):
        return {0: "f16", 1: "split"}[self._lib.wca_get_precision(self._h)]   # ("reference" is an alias of "split")

    def set_fuse_ln(self, on):
        """LayerNorm in the residual GEMMs' epilogue (needs the GPU to itself: wca.h) or as separate launches (the default)."""
        _lib.check(self._lib.wca_set_fuse_ln(self._h, 1 if on else 0))

    def set_overlap(self, on):
        """Phase 2 on its own stream (default) or everything on one stream (clean per-kernel profiles)."""
        _lib.check(self._lib.wca_set_overlap(self._h, 1 if on else 0))

    def set_decode_mode(self, fused=True, streams=1):
        """Few-row decoder GEMMs fused with LayerNorm / KV append / split-K (default) or separate launches. streams must be 1 (the
        two-stream form of the decode loop was removed; the library refuses anything else)."""
        _lib.check(self._lib.wca_set_decode_mode(self._h, 1 if fused else 0, int(streams)))

    def last_stage_ms(self):
        ms = (C.c_float * 8)()
        _lib.check(self._lib.wca_last_stage_ms(self._h, ms))
        return list(ms)
