"""csrc/conv_plan.h (tap tables, tap traits, data-gradient phase classes, pixel-shuffle map) against the definition of a
convolution: tests/conv_plan_check.cpp is a stand-alone host program that includes nothing but that header and sweeps
k in {1,2,3,5,7} x stride 1..4 x pad 0..3 x dil 1..2 x ih, iw 1..9 by brute force.  Built with the host compiler -- with
AddressSanitizer + UBSan where the toolchain has the runtimes (linked statically, so nothing has to be preloaded), plain otherwise."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "computervision.pytorch_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "conv_plan_check.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _host_compilers():
    names = [os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]
    return [p for p in (shutil.which(n) for n in names if n) if p]


def _build(out):
    """-> (command that built `out`, sanitized?)"""
    compilers = _host_compilers()
    assert compilers, "no host C++ compiler found (the HIP toolchain the build needs ships one)"
    log = []
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        for cxx in compilers:
            cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, SRC, "-o", out] + extra
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode == 0:
                return cmd, bool(extra)
            log.append(" ".join(cmd) + "\n" + r.stdout)
    raise AssertionError("conv_plan_check.cpp does not compile:\n" + "\n".join(log[-len(compilers):]))


def test_conv_plan_header_is_host_only():
    text = open(os.path.join(CSRC, "conv_plan.h")).read()
    includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', text)
    assert includes and all("hip" not in i and not i.endswith(".h") for i in includes), includes  # standard headers only
    assert "half_t" not in text and "__device__" not in text and "__global__" not in text


def test_conv_plan_against_the_definition(tmp_path):
    exe = str(tmp_path / "conv_plan_check")
    cmd, sanitized = _build(exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(("sanitized: " if sanitized else "plain: ") + " ".join(cmd))
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    m = re.search(r"conv_plan_check: (\d+) cases ok", r.stdout)
    assert m, r.stdout
    # every input pixel of every swept shape is one case: 5 kernels x 4 strides x 4 pads x 2 dilations x (1 + ... + 9)^2 pixels
    assert int(m.group(1)) >= 5 * 4 * 4 * 2 * 45 * 45
