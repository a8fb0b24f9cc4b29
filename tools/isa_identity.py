"""Compare the device code of two builds of libdpi_hip.so kernel by kernel, on the host (no GPU): the
sets of kernel symbols, every kernel's disassembly (llvm-objdump -d --no-show-raw-insn per symbol of the
unbundled gfx950 code objects, as tools/disasm.py) and build.kernel_resources' records.
usage: python tools/isa_identity.py <parent.so> <head.so> [summary.txt]"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from deeppicarditeration_amd import build  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(lib):
    """{symbol: disassembly text} over every gfx950 code object of `lib`."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fb = f"{d}/fb.bin"
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(lib), fb], check=True)
        data = Path(fb).read_bytes()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)]
        for k, st in enumerate(starts):
            part, co = f"{d}/p{k}.bin", f"{d}/c{k}.co"
            Path(part).write_bytes(data[st:starts[k + 1] if k + 1 < len(starts) else len(data)])
            r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}",
                                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True)
            if r.returncode:
                continue
            txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True,
                                 text=True, check=True).stdout
            cur = None
            for line in txt.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = m.group(1)
                    assert cur not in out, f"{cur} in two code objects"
                    out[cur] = []
                elif cur and line.strip():
                    # the instruction without its address column, which moves with the kernel's place in the object
                    out[cur].append(re.sub(r"\s*//\s*[0-9A-Fa-f]+:.*$", "", line).strip())
    return out


def main(parent, head, summary=None):
    a, b = kernels(parent), kernels(head)
    lines = [f"kernels: parent {len(a)}, head {len(b)}", f"only in parent: {sorted(set(a) - set(b))}",
             f"only in head: {sorted(set(b) - set(a))}"]
    differ = [k for k in sorted(set(a) & set(b)) if a[k] != b[k]]
    lines.append(f"instructions compared: {sum(len(v) for v in a.values())}")
    lines.append(f"kernels whose disassembly differs: {len(differ)} {differ[:20]}")
    key = lambda recs: sorted((r["mangled"], sorted(r.items())) for r in recs)  # noqa: E731
    ra, rb = key(build.kernel_resources(parent)), key(build.kernel_resources(head))
    lines.append(f"kernel_resources records: parent {len(ra)}, head {len(rb)}, equal: {ra == rb}")
    shared = {m for m, _ in ra} & {m for m, _ in rb}  # where one build drops or adds kernels
    lines.append(f"kernel_resources records of the {len(shared)} shared kernels equal: "
                 f"{[r for r in ra if r[0] in shared] == [r for r in rb if r[0] in shared]}")
    same = set(a) == set(b) and not differ and ra == rb
    lines.append("IDENTICAL" if same else "DIFFERENT")
    text = "\n".join(lines) + "\n"
    if summary:
        Path(summary).write_text(text)
    print(text, end="")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
