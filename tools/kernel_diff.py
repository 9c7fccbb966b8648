#!/usr/bin/env python3
"""Compare the gfx950 kernels of two source trees, without a GPU (and without torch).

    python tools/kernel_diff.py <parent tree> <candidate tree> [--jobs N] [--keep DIR] [--rename OLD=NEW ...]

Every HIP source of `han_amd/_lib.py:SOURCES` is compiled device-only in both trees with the flags
`_lib.build` uses, and every kernel symbol gets one line with a verdict:

  identical   the `llvm-objdump -d` text and encodings are equal once the address column is dropped
  equivalent  not identical, but the same .vgpr_count / .agpr_count / .group_segment_fixed_size /
              .private_segment_fixed_size / .vgpr_spill_count / .sgpr_spill_count in the code object's notes, the
              same occupancy in -Rpass-analysis=kernel-resource-usage, and the same number of each matrix
              (v_mfma*), global / buffer / flat / scratch, LDS (ds_*) and barrier opcode
  changed     anything else

Exit status 1 when the symbol sets differ, a tree yields no kernels, or any kernel is `changed`.  A refactor of
the kernel sources is gated on this: renamed registers or commuted operands pass, a changed resource or a
memory / matrix instruction more or less does not.

A kernel that the candidate renames (another template argument list, another name) is paired with `--rename OLD=NEW`
(repeatable): every OLD in a parent symbol (the mangled name, as printed) is replaced by NEW before the symbols are
paired, so the kernel gets a verdict instead of two "only in" lines.  Two parent kernels may end up paired with the
same candidate kernel, when one kernel has taken the place of both.
"""
import argparse
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

RESOURCE_KEYS = ("vgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                 "vgpr_spill_count", "sgpr_spill_count")
COUNTED = re.compile(r"^(v_mfma|v_smfmac|global_|buffer_|flat_|scratch_|ds_|s_barrier)")

_SYM = re.compile(r"^[0-9a-fA-F]+ <(.+)>:\s*$")
_ADDR = re.compile(r"//\s*[0-9A-Fa-f]+:\s*")
_TARGET = re.compile(r"\s*<[^<>\s]+\+0x[0-9A-Fa-f]+>\s*$")


def parse_disassembly(text):
    """`llvm-objdump -d` text -> {symbol: [instruction line without its address, ...]}.
    An instruction line reads `<tab>mnemonic operands   // ADDRESS: ENCODING ...`; the encoding stays.  What only
    restates where the code lies goes as well: the `<symbol+0xOFFSET>` that follows a branch (its encoding holds the
    relative target; the symbol differs for a renamed kernel) and the `...` lines of zero padding between symbols."""
    out, cur = {}, None
    for line in text.splitlines():
        m = _SYM.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        s = line.strip()
        if cur is None or not s or s == "..." or s.startswith("Disassembly of section") or "file format" in s:
            continue
        cur.append(" ".join(_TARGET.sub("", _ADDR.sub("// ", s)).split()))
    return out


def parse_notes(text):
    """`llvm-readelf --notes` text -> {kernel name: {key: int}} from the `amdhsa.kernels` list of the metadata."""
    out, lines = {}, text.splitlines()
    i = 0
    while i < len(lines) and lines[i].strip() != "amdhsa.kernels:":
        i += 1
    indent, cur = None, None
    for line in lines[i + 1:]:
        if not line.strip():
            continue
        m = re.match(r"^(\s*)(- )?\.([A-Za-z_]+):\s*(.*)$", line)
        lead = len(line) - len(line.lstrip())
        if indent is None:
            if not (m and m.group(2)):
                continue
            indent = lead
        if lead < indent:            # the list is over (amdhsa.target, amdhsa.version ...)
            break
        if m and m.group(2) and lead == indent:
            cur = {}
        if m and lead + (2 if m.group(2) else 0) == indent + 2 and cur is not None:
            key, val = m.group(3), m.group(4).strip().strip("'\"")
            if key == "name":
                out[val] = cur
            elif re.fullmatch(r"-?\d+", val):
                cur[key] = int(val)
    return out


_FN = re.compile(r"remark: Function Name: (\S+)")
_OCC = re.compile(r"remark:\s+Occupancy \[waves/SIMD\]: (\d+)")


def parse_occupancy(text):
    """stderr of -Rpass-analysis=kernel-resource-usage -> {function: waves per SIMD}."""
    out, cur = {}, None
    for line in text.splitlines():
        m = _FN.search(line)
        if m:
            cur = m.group(1)
            continue
        m = _OCC.search(line)
        if m and cur is not None:
            out[cur] = int(m.group(1))
    return out


def opcode_counts(stream):
    return Counter(op for op in (ln.split()[0] for ln in stream) if COUNTED.match(op))


def verdict(a, b):
    """a, b = (stream, resources, occupancy) of one kernel in the two trees."""
    if a[0] == b[0]:
        return "identical"
    same_res = all(a[1].get(k) == b[1].get(k) for k in RESOURCE_KEYS)
    if same_res and a[2] == b[2] and a[2] is not None and opcode_counts(a[0]) == opcode_counts(b[0]):
        return "equivalent"
    return "changed"


def pair_symbols(parent, candidate, renames=()):
    """-> (pairs, only_parent, only_candidate): pairs = sorted (parent symbol, candidate symbol) after the `renames`
    [(old, new), ...] have been applied, in order, to the parent's names; the rest of either side, sorted."""
    pairs, only_parent = [], []
    for k in sorted(parent):
        r = k
        for old, new in renames:
            r = r.replace(old, new)
        if r in candidate:
            pairs.append((k, r))
        else:
            only_parent.append(k)
    taken = {r for _, r in pairs}
    return pairs, only_parent, sorted(k for k in candidate if k not in taken)


def _tool(name):
    for cand in (shutil.which(name), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)):
        if cand and os.path.exists(cand):
            return cand
    raise SystemExit(f"{name} not found (PATH, $ROCM_PATH/llvm/bin)")


def _lib_of(tree):
    spec = importlib.util.spec_from_file_location("_han_lib_" + str(abs(hash(tree))), os.path.join(tree, "han_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)          # ctypes only: no torch, no library load
    return mod


def build_tree(tree, workdir, jobs):
    """-> {source: {kernel: (stream, resources, occupancy)}}"""
    lib = _lib_of(tree)
    os.makedirs(workdir, exist_ok=True)

    def one(src):
        obj = os.path.join(workdir, src.replace(".hip", ".co"))
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + list(lib.EXTRA_FLAGS.get(src, ())) + \
              ["--cuda-device-only", "--no-gpu-bundle-output", "-Rpass-analysis=kernel-resource-usage",
               "-c", os.path.join(tree, "han_amd", "csrc", src), "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stderr[-4000:])
        dis = subprocess.run([_tool("llvm-objdump"), "-d", obj], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([_tool("llvm-readelf"), "--notes", obj], capture_output=True, text=True, check=True).stdout
        streams, res, occ = parse_disassembly(dis), parse_notes(notes), parse_occupancy(r.stderr)
        return src, {k: (streams.get(k, []), res[k], occ.get(k)) for k in res}

    with ThreadPoolExecutor(max_workers=max(1, min(jobs, 16))) as ex:
        return dict(ex.map(one, lib.SOURCES))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("candidate")
    ap.add_argument("--jobs", type=int, default=8, help="parallel compiles (at most 16)")
    ap.add_argument("--keep", metavar="DIR", default=None, help="keep the code objects here")
    ap.add_argument("--rename", metavar="OLD=NEW", action="append", default=[],
                    help="replace OLD by NEW in the parent's symbol names before pairing (repeatable)")
    args = ap.parse_args(argv)
    if any("=" not in r for r in args.rename):
        ap.error("--rename takes OLD=NEW")
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    work = args.keep or tempfile.mkdtemp(prefix="kernel_diff_")
    try:
        pa = build_tree(os.path.abspath(args.parent), os.path.join(work, "parent"), args.jobs)
        ca = build_tree(os.path.abspath(args.candidate), os.path.join(work, "candidate"), args.jobs)
    finally:
        if not args.keep:
            shutil.rmtree(work, ignore_errors=True)
    bad = 0
    for src in sorted(set(pa) | set(ca)):
        p, c = pa.get(src, {}), ca.get(src, {})
        if not p or not c:
            print(f"{src}: no kernels in the {'parent' if not p else 'candidate'} tree")
            bad += 1
        pairs, only_p, only_c = pair_symbols(p, c, renames)
        for k in only_p:
            print(f"{src} {k}: only in the parent tree")
        for k in only_c:
            print(f"{src} {k}: only in the candidate tree")
        bad += len(only_p) + len(only_c)
        tally = Counter()
        for k, kc in pairs:
            v = verdict(p[k], c[kc])
            tally[v] += 1
            bad += v == "changed"
            extra = "" if v == "identical" else f"  instructions {len(p[k][0])} -> {len(c[kc][0])}"
            if v == "changed":
                diff = {key: (p[k][1].get(key), c[kc][1].get(key)) for key in RESOURCE_KEYS
                        if p[k][1].get(key) != c[kc][1].get(key)}
                if p[k][2] != c[kc][2]:
                    diff["occupancy"] = (p[k][2], c[kc][2])
                ops = {op: (opcode_counts(p[k][0])[op], opcode_counts(c[kc][0])[op])
                       for op in set(opcode_counts(p[k][0])) | set(opcode_counts(c[kc][0]))
                       if opcode_counts(p[k][0])[op] != opcode_counts(c[kc][0])[op]}
                extra += f"  {diff} {ops}"
            print(f"{src} {k}{'' if kc == k else ' -> ' + kc}: {v}{extra}")
        print(f"== {src}: {len(p)} kernels in the parent, {len(c)} in the candidate; "
              + ", ".join(f"{tally[v]} {v}" for v in ("identical", "equivalent", "changed")))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
