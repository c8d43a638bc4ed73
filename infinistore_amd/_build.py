"""In-tree native build for infinistore-amd.

Compiles the C++/HIP core with hipcc for gfx950 (MI355X) and links the
`_native` extension next to this file, so the built .so travels with the
repo snapshot (no JIT cache dependency). hipcc cross-compiles fine on a
machine with no GPU.
"""

import concurrent.futures
import os
import subprocess
import sys
import sysconfig
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "csrc"
PKG = REPO / "infinistore_amd"
BUILD = REPO / "build" / "native"

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("IFS_GFX_ARCH", "gfx950")

SOURCES = [
    CSRC / "core" / "log.cpp",
    CSRC / "core" / "protocol.cpp",
    CSRC / "core" / "mempool.cpp",
    CSRC / "gpu" / "gpu.hip",
    CSRC / "fabric" / "verbs_fabric.cpp",
    CSRC / "server" / "shard.cpp",
    CSRC / "server" / "kv_index.cpp",
    CSRC / "server" / "server.cpp",
    CSRC / "server" / "server_verbs.cpp",
    CSRC / "client" / "client.cpp",
    CSRC / "client" / "client_verbs.cpp",
    CSRC / "pybind.cpp",
]

HEADERS = sorted((CSRC).rglob("*.h")) + [Path(__file__)]


def _ext_suffix() -> str:
    return sysconfig.get_config_var("EXT_SUFFIX") or ".so"


def ext_path() -> Path:
    return PKG / f"_native{_ext_suffix()}"


def _pybind11_include() -> str:
    import pybind11

    return pybind11.get_include()


def _common_flags():
    return [
        "-O3",
        "-std=c++20",
        "-fPIC",
        "-D__HIP_PLATFORM_AMD__",
        f"-I{CSRC}",
        f"-I{_pybind11_include()}",
        f"-I{sysconfig.get_paths()['include']}",
        "-I/opt/rocm/include",
        "-Wall",
        "-Wno-unused-function",
    ]


def _needs_rebuild(obj: Path, src: Path) -> bool:
    if not obj.exists():
        return True
    omt = obj.stat().st_mtime
    if src.stat().st_mtime > omt:
        return True
    return any(h.stat().st_mtime > omt for h in HEADERS)


def _compile_one(src: Path) -> Path:
    rel = src.relative_to(CSRC).as_posix().replace("/", "_")
    obj = BUILD / (rel + ".o")
    if not _needs_rebuild(obj, src):
        return obj
    if src.suffix == ".hip":
        # Device code: hipcc for gfx950 only.
        cmd = [HIPCC, "-c", str(src), "-o", str(obj), f"--offload-arch={ARCH}"] + _common_flags()
    else:
        # Host-only C++ (no HIP headers included): plain g++ is much faster.
        cmd = ["g++", "-c", str(src), "-o", str(obj)] + _common_flags()
    print(f"  [{cmd[0].split('/')[-1]}]", src.relative_to(REPO))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError(f"compile failed: {src}")
    return obj


def build_native(force: bool = False, verbose: bool = True) -> Path:
    BUILD.mkdir(parents=True, exist_ok=True)
    out = ext_path()
    if force:
        for o in BUILD.glob("*.o"):
            o.unlink()
    with concurrent.futures.ThreadPoolExecutor(max_workers=os.cpu_count()) as ex:
        objs = list(ex.map(_compile_one, SOURCES))
    if out.exists() and all(o.stat().st_mtime <= out.stat().st_mtime for o in objs):
        return out
    cmd = [HIPCC, "-shared", "-o", str(out)] + [str(o) for o in objs] + ["-luv"]
    if verbose:
        print("  [link]", out.relative_to(REPO))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("link failed")
    return out


def ensure_native() -> None:
    """Build if the extension is missing or stale (imported by the package).

    Fast path: if the .so is newer than every source/header, skip without
    invoking any compiler (so a repo snapshot with a prebuilt .so — e.g. on a
    gpurun box — imports instantly)."""
    if os.environ.get("IFS_SKIP_BUILD"):
        return
    out = ext_path()
    if out.exists():
        omt = out.stat().st_mtime
        if all(s.stat().st_mtime <= omt for s in SOURCES + HEADERS):
            return
    try:
        build_native(verbose=False)
    except Exception as e:  # pragma: no cover - surfaced at import time
        raise ImportError(f"infinistore_amd native build failed: {e}") from e


if __name__ == "__main__":
    build_native(force="--force" in sys.argv)
