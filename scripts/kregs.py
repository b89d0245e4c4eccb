"""Per-kernel register use of a built library (CPU; reads the code objects' metadata).

    python scripts/kregs.py [lib.so] [name-filter]
    python scripts/kregs.py --compare old.so new.so

Prints VGPRs (arch + acc, as allocated), SGPRs, scratch bytes, spill counts,
LDS and code bytes per kernel, from the AMDHSA metadata note and the symbol
table of each gfx950 code object in the library's .hip_fatbin.  Waves per SIMD
follow from the VGPR total (512 per lane).  --compare matches the kernels of
two libraries by demangled name without the parameter list (parameter types
may change namespace; a trailing prefetch-depth argument 0 / 1 of k_fast_sums
is dropped) and prints every field that differs."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def code_objects(lib, tmp):
    fat = os.path.join(tmp, "fatbin.bin")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    data = open(fat, "rb").read()
    offs = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)] + [len(data)]
    out = []
    for k in range(len(offs) - 1):
        b = os.path.join(tmp, f"b{k}.bin")
        co = os.path.join(tmp, f"b{k}.co")
        open(b, "wb").write(data[offs[k]:offs[k + 1]])
        r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={b}", f"--output={co}"],
                           capture_output=True)
        if r.returncode == 0 and os.path.getsize(co):
            out.append(co)
    return out


def kernels(co):
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co],
                           capture_output=True, text=True, check=True).stdout
    cur = {}
    for line in notes.splitlines():
        s = line.strip().lstrip("- ")
        if ":" not in s:
            continue
        k, _, v = s.partition(":")
        k, v = k.strip(), v.strip()
        if k == ".agpr_count":          # first key of a kernel's map
            if cur.get(".name"):
                yield cur
            cur = {}
        cur[k] = v
    if cur.get(".name"):
        yield cur


def code_sizes(co):
    """function symbol -> its size in bytes (the kernel's code)"""
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", "--wide", co],
                          capture_output=True, text=True, check=True).stdout
    out = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            out[f[7]] = int(f[2], 0)
    return out


FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count",
          ".sgpr_spill_count", ".group_segment_fixed_size", ".max_flat_workgroup_size", "code")


def table(lib):
    """demangled kernel name without parameters -> its FIELDS"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            sizes = code_sizes(co)
            for k in kernels(co):
                k["code"] = sizes.get(k[".name"], -1)
                dm = subprocess.run(["c++filt", k[".name"]], capture_output=True, text=True).stdout.strip()
                dm = dm.replace("(anonymous namespace)::", "")
                m = re.match(r"^(?:void )?(.*?)\(", dm)
                name = re.sub(r"^(k_fast_sums<\d+, \d+), [01]>", r"\1>", m.group(1) if m else dm)
                out[name] = {f: str(k.get(f, "?")) for f in FIELDS}
    return out


def compare(old, new):
    a, b = table(old), table(new)
    print(f"kernels: {len(a)} -> {len(b)}")
    print("only in the first:", sorted(set(a) - set(b)))
    print("only in the second:", sorted(set(b) - set(a)))
    both = sorted(set(a) & set(b))
    differing = [n for n in both if a[n] != b[n]]
    for n in differing:
        print(n + ": " + ", ".join(f"{f.lstrip('.')} {a[n][f]} -> {b[n][f]}" for f in FIELDS if a[n][f] != b[n][f]))
    print(f"kernels in both: {len(both)}, differing: {len(differing)}")


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        return compare(sys.argv[2], sys.argv[3])
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "hyperdrive_amd", "_lib", "libhdverify.so")
    filt = sys.argv[2] if len(sys.argv) > 2 else ""
    with tempfile.TemporaryDirectory() as tmp:
        rows = []
        for co in code_objects(lib, tmp):
            sizes = code_sizes(co)
            for k in kernels(co):
                if filt in k[".name"]:
                    k["code"] = sizes.get(k[".name"], -1)
                    rows.append(k)
    for k in sorted(rows, key=lambda k: k[".name"]):
        v, a = int(k.get(".vgpr_count", 0)), int(k.get(".agpr_count", 0))
        tot = v + a if a == 0 else ((v + 3) // 4) * 4 + a
        print(f"{k['.name']} vgpr {v:3d} agpr {a:3d} total {tot:3d} waves/SIMD {min(8, 512 // max(tot, 1))}"
              f" sgpr {k.get('.sgpr_count', '?'):>3s} scratch {k.get('.private_segment_fixed_size', '?'):>4s}"
              f" vspill {k.get('.vgpr_spill_count', '?')} sspill {k.get('.sgpr_spill_count', '?')}"
              f" lds {k.get('.group_segment_fixed_size', '?'):>5s} code {k['code']:6d}"
              f" max_flat_wg {k.get('.max_flat_workgroup_size', '?')}")


if __name__ == "__main__":
    main()
