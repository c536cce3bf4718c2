"""Register / LDS / spill summary of the gfx950 kernels in built objects (CPU only).

    python tools/kstats.py [obj.o ...] [name-substring ...]
    python tools/kstats.py [obj.o ...] --asm MANGLED_NAME      (disassembly of one kernel)

Without objects: every face-vae_amd/csrc/build/conv*.o, one merged table.  Objects without device
code are skipped.
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


def main():
    args = sys.argv[1:]
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
