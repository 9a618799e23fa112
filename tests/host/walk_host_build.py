"""The recipe of the host programs of the two walks (baked_host.hip, occ_host.hip next to this file) and how they are run.

They are ordinary HIP programs that never launch: hipcc compiles the kernel sources they include for the host as well, and the
__host__ __device__ functions are called from main.  build() makes them in a directory of the caller's; sanitize=True adds
AddressSanitizer and UndefinedBehaviorSanitizer to the HOST side only -- the runtime clang links statically into the
executable; nothing is preloaded and nothing is loaded into Python.  run() starts a program as a child process that can open
no device."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PROGRAMS = ("baked_host", "occ_host")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


def hipcc():
    return shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc") or None


def build(out_dir, sanitize=False, timeout=300, names=PROGRAMS):
    """{name: path} of the programs, built into out_dir."""
    out = {}
    for name in names:
        exe = os.path.join(out_dir, name + ("_san" if sanitize else ""))
        cmd = [hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I",
               os.path.join(ROOT, "upnerf_amd", "csrc")] + (SANITIZE if sanitize else []) + [os.path.join(HERE, name + ".hip"), "-o", exe]
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=out_dir)
        if done.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed ({done.returncode}):\n{done.stderr[-4000:]}")
        out[name] = exe
    return out


def run(exe, directory, timeout=300):
    """Run a program on a directory of inputs with no device to open; (exit status, stderr)."""
    env = dict(os.environ, ROCR_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    done = subprocess.run([exe, directory], capture_output=True, text=True, timeout=timeout, env=env)
    return done.returncode, done.stderr
