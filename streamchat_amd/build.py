"""In-tree build of libstreamchat_hip.so (gfx950).  `python -m streamchat_amd.build`.

hipcc cross-compiles without a GPU, so this also is the CPU-side "does it build" check driven
by __graft_entry__.build().  The .so lands next to this file and travels to the GPU box with the
repo snapshot (it is git-ignored, not gpurun-ignored)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libstreamchat_hip.so")


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h")) or f == "Makefile"]
    srcs += [os.path.join(HERE, "..", "include", h) for h in ("streamchat_hip.h", "streamchat_hip_w8.h", "streamchat_hip_w8_batched.h", "streamchat_hip_kv8.h", "streamchat_hip_kv8_batched.h", "streamchat_hip_text.h")]
    return any(os.path.getmtime(s) > t for s in srcs)


def build(force: bool = False, jobs: int = 0) -> str:
    if force:
        subprocess.check_call(["make", "-s", "-C", CSRC, "clean"])
    if force or needs_build():
        # MAX_JOBS when set, else the CPUs this process may run on; at most 16 (os.cpu_count() counts the whole machine's)
        j = jobs or min(16, int(os.environ.get("MAX_JOBS") or 0) or len(os.sched_getaffinity(0)))
        subprocess.check_call(["make", "-s", f"-j{j}", "-C", CSRC])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
