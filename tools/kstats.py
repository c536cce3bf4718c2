"""Register / LDS / spill summary of the gfx950 kernels in built objects (CPU only).

    python tools/kstats.py [obj.o ...] [name-substring ...]
    python tools/kstats.py [obj.o ...] --asm MANGLED_NAME      (disassembly of one kernel)
    python tools/kstats.py --compare DIR_A DIR_B [glob]        (two build directories, default glob conv*.o)

Without objects: every face-vae_amd/csrc/build/conv*.o, one merged table.  Objects without device
code are skipped.

--compare is the check of a kernel-neutral refactor: it lists the kernels only in A, only in B,
those whose register / LDS / spill / private-segment figures differ and those whose disassembly
differs, and exits non-zero on any difference.  Kernels are matched on the demangled name without
"(anonymous namespace)::" (a kernel or an argument struct may move in or out of one); the
disassembly is compared without addresses, encodings, branch-target annotations and the
pc-relative distance to a global (the literal of the s_add_u32 / s_addc_u32 pair on the registers
an s_getpc_b64 just wrote; nothing else near an s_getpc_b64 is touched).
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_on_co(obj, *cmds):
    """Outputs of each cmd on obj's gfx950 code object, unbundled once; None if obj has none."""
    sections = subprocess.run([f"{LLVM}/llvm-readelf", "-S", obj], capture_output=True, text=True, check=True).stdout
    if ".hip_fatbin" not in sections:
        return None
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fb.bin"), os.path.join(d, "k.co")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(d, "x.o")], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={fb}", f"--output={co}", "--unbundle"], check=True)
        return [subprocess.run(c + [co], capture_output=True, text=True, check=True).stdout for c in cmds]


def notes(obj):
    out = _run_on_co(obj, [f"{LLVM}/llvm-readelf", "--notes"])
    return out[0] if out else ""


FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
           "private_segment_fixed_size", "group_segment_fixed_size")


def _kernels(build_dir, pattern):
    """{matching name: (figures, normalised disassembly)} of every kernel in build_dir's objects."""
    raw, demangled = {}, {}
    for obj in sorted(glob.glob(os.path.join(build_dir, pattern))):
        out = _run_on_co(obj, [f"{LLVM}/llvm-readelf", "--notes"], [f"{LLVM}/llvm-objdump", "-d"],
                         [f"{LLVM}/llvm-objdump", "-t"], [f"{LLVM}/llvm-objdump", "-t", "-C"])
        if not out:
            continue
        # the symbol table plain and demangled, line for line: "... <tab>SIZE NAME" (this LLVM ships no
        # llvm-cxxfilt, and binutils' c++filt does not know the bf16 mangling DF16b)
        plain_t, nice_t = out[2].split("\n"), out[3].split("\n")
        if len(plain_t) != len(nice_t):
            sys.exit(f"{obj}: llvm-objdump -t and -t -C list {len(plain_t)} and {len(nice_t)} lines")
        for plain, nice in zip(plain_t, nice_t):
            if "\t" in plain:
                demangled[plain.split("\t")[-1].split(" ", 1)[1].replace(".protected ", "")] = \
                    nice.split("\t")[-1].split(" ", 1)[1].replace(".protected ", "")
        body, sym = {}, None
        for line in out[1].split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                sym = m.group(1)
                body[sym] = []
            elif sym and line.startswith("\t"):
                ins = line.split("//")[0].strip()                   # drops address, encoding, <target+off>
                # s_getpc_b64 s[L:H]; s_add_u32 sL, sL, lit; s_addc_u32 sH, sH, lit: the distance to a
                # global (an address).  Only that pair, on the registers the s_getpc_b64 wrote.
                for back, op in ((1, "s_add_u32 s{0}, s{0}, "), (2, "s_addc_u32 s{1}, s{1}, ")):
                    m = len(body[sym]) >= back and re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]$", body[sym][-back])
                    if m and ins.startswith(op.format(*m.groups())):
                        ins = re.sub(r"(0x[0-9a-f]+|\d+)$", "<pcrel>", ins)
                body[sym].append(ins)
        for blk in out[0].split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            fig = {k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1] for k in FIGURES}
            fig["agpr_count"] = blk.split("\n")[0].strip()
            text = body.get(name, [])
            while text and text[-1] in ("s_code_end", "s_nop 0", "..."):  # padding behind s_endpgm
                text.pop()
            raw[name] = (fig, text)
    res = {}
    for n in raw:
        if n not in demangled:
            sys.exit(f"kernel {n} of the metadata notes is not in the symbol table")
        key = demangled[n].replace("(anonymous namespace)::", "")
        if key in res:
            sys.exit(f"two kernels match as {key}")
        res[key] = raw[n]
    return res


def compare(dir_a, dir_b, pattern="conv*.o"):
    a, b = _kernels(dir_a, pattern), _kernels(dir_b, pattern)
    if not a or not b:
        sys.exit(f"no kernels in {dir_a if not a else dir_b}/{pattern}")
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    both = sorted(set(a) & set(b))
    figs = [k for k in both if a[k][0] != b[k][0]]
    asm = [k for k in both if a[k][1] != b[k][1]]
    empty = [k for k in both if not a[k][1] or not b[k][1]]
    for title, ks in (("only in A", only_a), ("only in B", only_b), ("figures differ", figs),
                      ("disassembly differs", asm), ("no disassembly found", empty)):
        print(f"{title}: {len(ks)}")
        for k in ks:
            print("   ", k)
            if title == "figures differ":
                print("       ", {f: (a[k][0][f], b[k][0][f]) for f in FIGURES if a[k][0][f] != b[k][0][f]})
    print(f"kernels: {len(a)} in A, {len(b)} in B, {len(both)} in both")
    return 1 if only_a or only_b or figs or asm or empty else 0


def main():
    args = sys.argv[1:]
    if args and args[0] == "--compare":
        if len(args) not in (3, 4):
            sys.exit("usage: kstats.py --compare DIR_A DIR_B [glob]")
        sys.exit(compare(*args[1:]))
    objs = []
    while args and args[0].endswith(".o"):
        objs.append(args.pop(0))
    if not objs:
        objs = sorted(glob.glob(os.path.join(ROOT, "face-vae_amd", "csrc", "build", "conv*.o")))
    if args and args[0] == "--asm":
        for obj in objs:
            out = _run_on_co(obj, [f"{LLVM}/llvm-readelf", "--notes"],
                             [f"{LLVM}/llvm-objdump", "-d", f"--disassemble-symbols={args[1]}"])
            if out and args[1] in out[0]:
                print(out[1])
                return
        sys.exit(f"kernel {args[1]} not found in {len(objs)} object(s)")
    for obj in objs:
        for blk in notes(obj).split("  - .agpr_count:")[1:]:
            m = re.search(r"\.name:\s+(\S+)", blk)
            if not m or (args and not any(a in m.group(1) for a in args)):
                continue
            g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
            print(f"{m.group(1)[:90]:90s} vgpr {g('vgpr_count'):>3} agpr {blk.split(chr(10))[0].strip():>3} "
                  f"spill {g('vgpr_spill_count'):>3} sgpr {g('sgpr_count'):>3}/{g('sgpr_spill_count'):>3} priv {g('private_segment_fixed_size'):>4} lds {g('group_segment_fixed_size')}")


if __name__ == "__main__":
    main()
