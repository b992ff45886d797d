"""Per-kernel register, scratch, LDS and occupancy figures of two source trees side by side, as the compiler reports them
(-Rpass-analysis=kernel-resource-usage).  No device is needed.

    python tools/kernel_resources.py --parent <checkout of the parent>/computervision.pytorch_amd/csrc nms.hip tiles.hip ... [--out FILE]

Exit status 1 when a kernel gained scratch, changed its LDS size or lost occupancy; a register count that moves is only shown."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "computervision.pytorch_amd", "csrc")
FIELDS = [("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "LDS"),
          ("Occupancy [waves/SIMD]", "waves")]


def resources(path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", path,
           "-o", os.devnull]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise SystemExit(f"hipcc failed on {path}:\n{r.stdout}")
    out, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass", line)
        if m and name is not None:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def demangle(names):
    """The kernel's own name and integer template arguments out of the Itanium name (kernels live in anonymous namespaces here)."""
    out = {}
    for n in names:
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", n) or re.match(r"_Z(\d+)", n)
        if not m:
            out[n] = n
            continue
        end = m.end() + int(m.group(1))
        t = re.match(r"I((?:L[a-z]\d+E)+)E", n[end:])
        out[n] = n[m.end():end] + ("<" + ", ".join(re.findall(r"L[a-z](\d+)E", t.group(1))) + ">" if t else "")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent commit's csrc directory")
    ap.add_argument("--out")
    ap.add_argument("files", nargs="+")
    args = ap.parse_args()
    lines = ["kernel resources, gfx950, -O3: parent | new   (SGPRs, VGPRs, scratch bytes/lane, LDS bytes/block, waves/SIMD)",
             f"{'file':22s} {'kernel':44s} " + " ".join(f"{s:>13s}" for _, s in FIELDS) + "  note"]
    bad = 0
    for f in args.files:
        # keyed by the kernel's own name and template integers: a renamed argument type changes the mangled name, not the kernel
        old, new = ({name: v for name, v in ((demangle([k])[k], v) for k, v in resources(path).items())}
                    for path in (os.path.join(args.parent, f), os.path.join(CSRC, f)))
        names = {k: k for k in set(old) | set(new)}
        for k in sorted(names):
            a, b = old.get(k), new.get(k)
            if a is None or b is None:
                lines.append(f"{f:22s} {names[k]:44s} only in the {'new' if a is None else 'parent'} build")
                bad += 1
                continue
            note = []
            if b[FIELDS[2][0]] > a[FIELDS[2][0]]:
                note.append("SCRATCH GREW")
            if b[FIELDS[3][0]] != a[FIELDS[3][0]]:
                note.append("LDS DIFFERS")
            if b[FIELDS[4][0]] < a[FIELDS[4][0]]:
                note.append("OCCUPANCY FELL")
            bad += len(note)
            if not note and any(a[key] != b[key] for key, _ in FIELDS):
                note.append("registers moved")
            lines.append(f"{f:22s} {names[k]:44s} " + " ".join(f"{a[key]:>6d}|{b[key]:<6d}" for key, _ in FIELDS) + "  " + ", ".join(note))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text, end="")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
