#!/usr/bin/env python3
"""Compares the gfx950 code of the kernels in two builds of the library, kernel by kernel: resources from the code object's metadata
notes (.vgpr_count, .sgpr_count, LDS, scratch, kernarg size) and the instruction sequence from llvm-objdump. Scalar loads whose only
difference is the immediate offset are counted apart (the kernarg layout of a struct argument that lost fields), everything else is
printed; a kernel whose instructions differ only in register numbers is reported as REGISTERS. Kernels are paired by demangled name after RENAME (regex -> replacement, applied to the OLD build's names).
  python tools/kernel_diff.py OLD_BUILD_DIR NEW_BUILD_DIR [name-filter]      (BUILD_DIR: whisper-char-alignment_amd/build of a tree)"""
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")
# template parameters dropped from the product kernels: the s_memtime stamp switch and the unadopted VALU row-sum attention form
RENAME = [(r"(gemm256p_f16_kernel<[^,]+, [^,]+, [^,]+), 0, ", r"\1, "),
          (r"attn_kernel<(true|false), (true|false), false>", r"attn_kernel<\1, \2>"),
          (r"attn32_kernel<false, false>", "attn32_kernel"),
          # kernels that gained a per-row instance (wca_decode with per_row 1): the uniform launches take the <..., false> ones
          (r"(gemm_rows_f16_kernel<[^,]+, [^,]+, [^,>]+)>", r"\1, false>"),
          (r"\b(attn_decode_kernel|decode_select_kernel)\(", r"\1<false>("),
          # the waves per workgroup of the pair attention: a constant of the body now (only 4 was ever instantiated)
          (r"attn_split_kernel<(true|false), (true|false), 4>", r"attn_split_kernel<\1, \2>")]
SLOAD = re.compile(r"^(s_load_\w+|s_buffer_load_\w+)\s+(.*),\s*(0x[0-9a-fA-F]+|\d+)$")
REG = re.compile(r"\b([vsa])(\d+|\[\d+:\d+\])")
ZERO_DWORD = "v_cndmask_b32_e32 v0, s0, v0, vcc"   # what llvm-objdump prints for 0x00000000


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def code_object(obj, tmp):
    fat, co = os.path.join(tmp, "k.fatbin"), os.path.join(tmp, os.path.basename(obj) + ".co")
    subprocess.check_call([LLVM + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([LLVM + "clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                           "--output=" + co, "--unbundle"])
    return co


def kernels(obj, tmp):
    """{demangled name: (resources dict, [instructions])}"""
    co = code_object(obj, tmp)
    notes = subprocess.run([LLVM + "llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    res = {}
    for ent in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        m = re.search(r"\.name:\s+(\S+)", ent)
        res[m.group(1)] = {k: (re.search(r"\.%s:\s+(\S+)" % k, ent) or [None, "?"])[1] for k in KEYS}
    dis = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    code, cur = {}, None
    for line in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1)
            code[cur] = []
            continue
        ins = re.sub(r"\s*//.*$", "", line).strip()
        ins = re.sub(r"\s*<[^>]*>$", "", ins)   # branch target labels carry absolute addresses
        if cur and ins and ins != "...":   # (a run of zero padding after s_endpgm: its presence depends on where the next kernel starts)
            code[cur].append(re.sub(r"\s+", " ", ins))
    for ins in code.values():   # a single zero dword of padding behind the last s_endpgm decodes as an instruction; like the longer runs, it is layout
        while len(ins) > 1 and ins[-1] == ZERO_DWORD and ins[-2] in (ZERO_DWORD, "s_endpgm"):
            ins.pop()
    names = demangle(sorted(res))
    return {names[k]: (res[k], code.get(k, [])) for k in res}


def rename(name):
    name = re.sub(r"^void ", "", name)   # (c++filt prints the return type of template instances only)
    for pat, rep in RENAME:
        name = re.sub(pat, rep, name)
    return name


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    flt = sys.argv[3] if len(sys.argv) > 3 else ""
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for new_obj in sorted(glob.glob(os.path.join(new_dir, "*.o"))):
            old_obj = os.path.join(old_dir, os.path.basename(new_obj))
            if not os.path.exists(old_obj) or subprocess.run([LLVM + "llvm-readelf", "-S", new_obj], capture_output=True, text=True).stdout.find(".hip_fatbin") < 0:
                continue
            new = {re.sub(r"^void ", "", k): v for k, v in kernels(new_obj, tmp).items()}
            old = {rename(k): v for k, v in kernels(old_obj, tmp).items()}
            only_old = sorted(set(old) - set(new))
            only_new = sorted(set(new) - set(old))
            same = sload = regs_only = 0
            for name in sorted(set(old) & set(new)):
                if flt not in name:
                    continue
                (ro, co), (rn, cn) = old[name], new[name]
                diffs = ["%s %s -> %s" % (k, ro[k], rn[k]) for k in KEYS if ro[k] != rn[k] and k != "kernarg_segment_size"]
                n_sload = n_reg = 0
                if len(co) != len(cn):
                    diffs.append("instruction count %d -> %d" % (len(co), len(cn)))
                    diffs += list(difflib.unified_diff(co, cn, lineterm="", n=1))[:40]
                else:
                    for a, b in zip(co, cn):
                        if a == b:
                            continue
                        ma, mb = SLOAD.match(a), SLOAD.match(b)
                        if ma and mb and ma.group(1, 2) == mb.group(1, 2):
                            n_sload += 1
                        elif REG.sub(r"\1#", a) == REG.sub(r"\1#", b):
                            n_reg += 1
                        else:
                            diffs.append("  %s  ->  %s" % (a, b))
                sload += n_sload
                if n_reg and not diffs:
                    # same opcodes, operands and immediates; only the register numbers differ
                    regs_only += 1
                    print("  REGISTERS %s: %d of %d instructions name other registers (%s -> %s VGPRs)" % (name, n_reg, len(cn), ro["vgpr_count"], rn["vgpr_count"]))
                elif diffs:
                    bad += 1
                    print("DIFF %s: %s\n    %s" % (os.path.basename(new_obj), name, "\n    ".join(diffs[:60])))
                else:
                    same += 1
                    if ro["kernarg_segment_size"] != rn["kernarg_segment_size"] or n_sload:
                        print("  kernarg %s: %s -> %s bytes, %d scalar-load offsets" % (name, ro["kernarg_segment_size"], rn["kernarg_segment_size"], n_sload))
            print("%-22s %4d kernels identical (%d scalar-load offsets moved), %d differ in register assignment only, %d only in old, %d only in new" % (
                os.path.basename(new_obj), same, sload, regs_only, len(only_old), len(only_new)))
            for k in only_old:
                print("    only old: " + k)
            for k in only_new:
                print("    only new: " + k)
    print("kernels with other differences:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
