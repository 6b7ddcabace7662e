"""CPU tests of the drop-in boundary: libwca.so loads without a GPU and exports every symbol that
include/wca.h declares, with a ctypes signature for each (no compute calls here)."""
import ctypes
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "wca.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(wca_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_hot_path():
    names = _declared()
    for need in ["wca_log_mel", "wca_get_attentions", "wca_median_filter", "wca_filter_attention", "wca_force_align", "wca_dtw",
                 "wca_align_batch", "wca_engine_create", "wca_engine_destroy", "wca_load_weight"]:
        assert need in names


def test_library_exports_every_declared_symbol(wca):
    lib = wca._lib.load()
    for name in _declared():
        assert hasattr(lib, name), "libwca.so does not export %s" % name
        assert name in wca._lib.SIGNATURES, "no ctypes signature for %s" % name
    assert set(wca._lib.SIGNATURES) == set(_declared())
    assert lib.wca_version() >= 1
    assert isinstance(lib.wca_last_error(), (bytes, type(None)))


def test_removed_cu_partition_is_not_exported(wca):
    """The CU-partition experiment left the library: no symbol, no declaration, no binding (an old caller fails at load, not at run time)."""
    lib = wca._lib.load()
    assert not hasattr(lib, "wca_set_cu_partition")
    assert "wca_set_cu_partition" not in _declared() and "wca_set_cu_partition" not in wca._lib.SIGNATURES
    assert not hasattr(wca.WhisperAMD, "set_cu_partition")


def test_removed_decode_and_alignment_names_are_not_exported(wca):
    """One descriptor call each replaced the four decode and the seven fused-alignment entry points: the ten names that left are in no
    symbol table, declaration or binding."""
    lib = wca._lib.load()
    header = open(os.path.join(ROOT, "include", "wca.h")).read()
    for name in ("wca_greedy_decode", "wca_greedy_decode_ex", "wca_greedy_decode_rows", "wca_decode_rows_sampled", "wca_decode_opts_ex",
                 "wca_align_batch_enqueue_ex", "wca_align_batch_enqueue_open", "wca_align_batch_fetch_ex", "wca_align_batch_fetch_open"):
        assert not hasattr(lib, name), name
        assert name not in header and name not in wca._lib.SIGNATURES, name
    assert not hasattr(wca._lib, "DecodeOptsEx")
    assert {"wca_decode", "wca_align_batch", "wca_align_batch_enqueue", "wca_align_batch_fetch"} <= set(_declared())


def test_descriptor_calls_refuse_null_arguments_without_a_gpu(wca):
    """wca_decode and the three fused-alignment calls: no engine and no descriptor, and no engine with an empty descriptor, are refused with
    a message that says `null` before any HIP call; the ctypes descriptors have the header's layout."""
    lib, L = wca._lib.load(), wca._lib
    dd, ad, ar = L.DecodeDesc(), L.AlignDesc(), L.AlignResult()
    calls = [(lib.wca_decode, (None, None)), (lib.wca_decode, (None, ctypes.byref(dd))),
             (lib.wca_align_batch_enqueue, (None, None)), (lib.wca_align_batch_enqueue, (None, ctypes.byref(ad))),
             (lib.wca_align_batch_fetch, (None, 0, 0, 0, None)), (lib.wca_align_batch_fetch, (None, 0, 0, 0, ctypes.byref(ar))),
             (lib.wca_align_batch, (None, None, None)), (lib.wca_align_batch, (None, ctypes.byref(ad), ctypes.byref(ar)))]
    for fn, args in calls:
        assert lib.wca_test_set_switch(b"no_such_switch", 1) < 0 and b"null" not in lib.wca_last_error()
        assert fn(*args) < 0 and b"null" in lib.wca_last_error(), (fn.__name__, args)
    # pointers, then 64-bit fields, then 32-bit fields, padded to the 8-byte alignment of the pointers
    assert ctypes.sizeof(dd) == 16 * 8 + 1 * 8 + 4 * 4
    assert ctypes.sizeof(ad) == 7 * 8 + 1 * 8 + 3 * 4 + 4
    assert ctypes.sizeof(ar) == 5 * 8
    header = open(os.path.join(ROOT, "include", "wca.h")).read()
    for name, struct in (("wca_decode_desc", L.DecodeDesc), ("wca_align_desc", L.AlignDesc), ("wca_align_result", L.AlignResult)):
        body = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, header, flags=re.S).group(1)
        assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f[0] for f in struct._fields_], name


def test_struct_layouts_match_header(wca):
    assert ctypes.sizeof(wca._lib.ModelDims) == 10 * 4
    assert ctypes.sizeof(wca._lib.AlignOpts) == 8 * 4
    assert [f[0] for f in wca._lib.AlignOpts._fields_] == ["aggregation", "topk", "w_colnorm", "w_rownorm", "w_coverage", "sot_len",
                                                          "medfilt_width", "qk_scale"]


def test_null_engine_is_an_error_not_a_crash(wca):
    lib = wca._lib.load()
    assert lib.wca_engine_synchronize(None) < 0
    assert b"null" in lib.wca_last_error()
    assert lib.wca_finalize_weights(None) < 0
    # every entry point of the alignment and the audio file that takes an engine checks its arguments before its first HIP call: a null
    # engine with null / zero arguments is refused on a machine without a GPU
    names = []
    for f in ("engine_align.hip", "engine_audio.hip"):
        src = open(os.path.join(ROOT, "whisper-char-alignment_amd", "csrc", f)).read()
        names += re.findall(r"^int (wca_\w+)\(wca_engine\* e\b", src, flags=re.M)
    assert len(names) >= 22 and {"wca_log_mel", "wca_resample_16k", "wca_align_batch_fetch", "wca_probe_strict_tp"} <= set(names)
    for name in names:
        args = [None if issubclass(t, ctypes._Pointer) or t is ctypes.c_void_p else 0 for t in wca._lib.SIGNATURES[name][1]]
        assert lib.wca_test_set_switch(b"no_such_switch", 1) < 0 and b"null" not in lib.wca_last_error()
        assert getattr(lib, name)(*args) < 0, name
        assert b"null" in lib.wca_last_error(), name


def test_library_is_in_tree_and_has_gfx950_code(wca):
    path = wca._lib.LIB_PATH
    assert path.startswith(ROOT) and os.path.exists(path)
    blob = open(path, "rb").read()
    assert b"gfx950" in blob and b"gemm_f16_kernel" in blob and b"dtw_kernel" in blob and b"attn_kernel" in blob


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "whisper-char-alignment_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), "%s imports the oracle" % f
                assert "liboracle" not in text


def test_switch_table_reads_no_environment_and_rejects_removed_names(wca):
    """The test switches of the library (csrc/debug_switch.cpp, wca_test_set_switch: no environment variable sets them) and
    the round-5 null-argument paths, none of which needs a GPU."""
    lib = wca._lib.load()
    for name in (b"attn_split_variant", b"head_stats_general", b"fail_precision_alloc", b"attn_split_drop", b"gemm_ring"):
        assert lib.wca_test_set_switch(name, 1) == 0 and lib.wca_test_set_switch(name, 0) == 0
    assert lib.wca_test_set_switch(b"no_such_switch", 1) < 0 and b"unknown switch" in lib.wca_last_error()
    for name in (b"attn_variant", b"gemm_supertile", b"ln_pair_v4"):   # removed A/B overrides
        assert lib.wca_test_set_switch(name, 1) < 0 and b"unknown switch" in lib.wca_last_error()
    assert lib.wca_test_set_switch(None, 1) < 0
    assert lib.wca_test_set_attn_split_drop(5) < 0 and lib.wca_test_set_attn_split_drop(9) == 0 and lib.wca_test_set_attn_split_drop(0) == 0
    assert lib.wca_weights_inexact(None, None, None, None, 0) < 0 and lib.wca_set_allow_rounded_weights(None, 1) < 0
    # the strided kernel-level entry points refuse null arguments before their first HIP call: no engine, no description, no plan slot, no operands
    gd, ad, plan = wca._lib.GemmDesc(), wca._lib.AttnDesc(), (ctypes.c_int32 * 2)(-1, -1)
    for args in ((None, None, None), (None, ctypes.byref(gd), plan)):
        assert lib.wca_test_set_switch(b"no_such_switch", 1) < 0 and b"null" not in lib.wca_last_error()
        assert lib.wca_test_gemm_ex(*args) < 0 and b"null" in lib.wca_last_error() and list(plan) == [-1, -1]
    for args in ((None, None), (None, ctypes.byref(ad))):
        assert lib.wca_test_set_switch(b"no_such_switch", 1) < 0 and b"null" not in lib.wca_last_error()
        assert lib.wca_test_attention_ex(*args) < 0 and b"null" in lib.wca_last_error()
    header = open(os.path.join(ROOT, "include", "wca.h")).read()
    body = re.search(r"typedef struct wca_test_gemm_desc \{([^{}]*)\} wca_test_gemm_desc;", header, flags=re.S).group(1)
    names = [n for decl in re.findall(r"([\w ,*]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) for n in re.findall(r"(\w+)\s*(?:,|$)", decl)]
    assert names == [f[0] for f in wca._lib.GemmDesc._fields_] and names[-4:] == ["ln_gamma", "ln_beta", "ln_out", "ln_ld"]
    rd = wca._lib.GemmRowsDesc()
    for args in ((None, None), (None, ctypes.byref(rd))):
        assert lib.wca_test_set_switch(b"no_such_switch", 1) < 0 and b"null" not in lib.wca_last_error()
        assert lib.wca_test_gemm_rows_ex(*args) < 0 and b"null" in lib.wca_last_error()
    # the decoder's dispatch plan is host arithmetic: no output slot, or no shape, is refused
    slots = (ctypes.c_int64 * 8)(*([-1] * 8))
    assert lib.wca_test_dec_gemm_plan(1024, 1, 1024, 1024, 0, 0, None) < 0 and b"null" in lib.wca_last_error()
    assert lib.wca_test_dec_gemm_plan(1024, 0, 1024, 1024, 0, 0, slots) < 0 and b"bad shape" in lib.wca_last_error() and list(slots) == [-1] * 8
    # the descriptions mirror the header's structs: 6 pointers, then the 64-bit strides, then the 32-bit fields (the GEMM's: then the three
    # LayerNorm pointers of out_mode 3 and ln_ld, padded to the pointers' alignment)
    assert ctypes.sizeof(gd) == 6 * 8 + 4 * 8 + 16 * 4 + 3 * 8 + 4 + 4 and ctypes.sizeof(ad) == 6 * 8 + 10 * 8 + 13 * 4 + 4
    assert ctypes.sizeof(rd) == 10 * 8 + 8 + 14 * 4
    # the library reads no environment variable on a launch path or in the switch table: the remaining getenv calls are one-time initialisers
    for f in ("gemm.hip", "attention.hip", "attention_split.hip", "postproc.hip", "elementwise.hip", "gemm_rows.hip", "dtw.hip", "logmel.hip", "decode.hip",
              "debug_switch.cpp"):
        assert "getenv" not in open(os.path.join(ROOT, "whisper-char-alignment_amd", "csrc", f)).read(), f
