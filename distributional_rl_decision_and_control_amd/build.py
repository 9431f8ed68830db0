"""Build the gfx950 libraries in-tree (hipcc cross-compiles; no GPU needed).

    python -m distributional_rl_decision_and_control_amd.build [--force]

lib/libasvrl.so      the product: learner kernels with bf16 MFMA operands, f32 accumulation
lib/libasvrl_f32.so  the same sources with ASVRL_OPERAND_F32=1: every learner operand, weight image
                     and saved activation f32 (v_mfma_f32_32x32x2_f32), the parity build that pins
                     the hand-written learner to the reference's fp32 arithmetic
Sources compile to objects in parallel (lib/obj/), then each variant links once.
"""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCES = [os.path.join(HERE, "csrc", f) for f in ("asvrl_env.hip", "asvrl_learn.hip", "asvrl_critic.hip", "asvrl_critic_fused.hip",
                                                             "asvrl_optim.hip", "asvrl_wgrad.hip", "asvrl_mlp.hip",
                                                             "asvrl_per.hip", "asvrl_rainbow.hip", "asvrl_rainbow_net.hip",
                                                             "asvrl_eval.hip", "asvrl_dqn.hip", "asvrl_ddpg.hip",
                                                             "asvrl_sac.hip", "asvrl_noise.hip")]
HEADERS = [os.path.join(HERE, "csrc", "asvrl_common.h"), os.path.join(HERE, "csrc", "asvrl_mfma.h"),
           os.path.join(HERE, "csrc", "asvrl_lds.h"), os.path.join(HERE, "csrc", "asvrl_vonmises_k1.h"),
           os.path.join(HERE, "csrc", "asvrl_critic_tile.h"), os.path.join(HERE, "csrc", "asvrl_actor_tile.h"),
           os.path.join(HERE, "csrc", "asvrl_dqn_tile.h"), os.path.join(HERE, "csrc", "asvrl_ddpg_tile.h"),
           os.path.join(HERE, "csrc", "asvrl_sac_tile.h"), os.path.join(HERE, "csrc", "asvrl_rs_stream.h"),
           os.path.join(ROOT, "include", "asvrl.h")]
OUT = os.path.join(HERE, "lib", "libasvrl.so")
OUT_F32 = os.path.join(HERE, "lib", "libasvrl_f32.so")
VARIANTS = {OUT: [], OUT_F32: ["-DASVRL_OPERAND_F32=1"]}
# per-source flags: the fused critic keeps its persistent weight-gradient accumulators in AGPRs (inline
# asm) and every other MFMA in the VGPR form; no NaN operands on the path (ReLU as one v_max_f32, no
# canonicalising max). The f32 build drops the VGPR form: it has no inline-asm accumulators, and the
# compiler's own AGPR placement spills far less there.
SOURCE_FLAGS = {"asvrl_critic_fused.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1", "-fno-honor-nans"]}
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("ASVRL_OFFLOAD_ARCH", "gfx950")

# -ffp-contract=off: the env kernel reproduces the reference's f64 operation order; FMA
# contraction would change rounding (the masks are compared bit-exactly).
FLAGS = ["-O3", f"--offload-arch={ARCH}", "-fPIC", "-std=c++17", "-ffp-contract=off",
         "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "include")]


def _sig(cmd):
    """Signature of one compile: the full command (compiler, arch, every flag, the source) and this file's
    own text, so a change of HIPCC, ASVRL_OFFLOAD_ARCH, FLAGS / SOURCE_FLAGS or build.py rebuilds."""
    h = hashlib.sha1(" ".join(c for c in cmd if not c.endswith(".tmp")).encode())
    with open(os.path.abspath(__file__), "rb") as f:
        h.update(f.read())
    return h.hexdigest()


def _obj_fresh(o, src, hdr_t, sig):
    if not os.path.exists(o) or os.path.getmtime(o) < max(os.path.getmtime(src), hdr_t):
        return False
    try:
        with open(o + ".sig") as f:
            return f.read().strip() == sig
    except OSError:
        return False


def stale(out):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    if any(os.path.getmtime(f) > t for f in SOURCES + HEADERS):
        return True
    try:   # the link's signature: the objects' signatures in order
        with open(out + ".sig") as f:
            return f.read().strip() != _link_sig(out)
    except OSError:
        return True


def _obj(out, src):
    return os.path.join(os.path.dirname(out), "obj", os.path.basename(out) + "." + os.path.basename(src) + ".o")


def _compile_cmd(out, src, extra):
    sf = SOURCE_FLAGS.get(os.path.basename(src), [])
    if extra:   # the f32 build: its accumulators are plain MFMA results (no AGPR pinning)
        sf = [f for f in sf if f not in ("-mllvm", "-amdgpu-mfma-vgpr-form=1")]
    o = _obj(out, src)
    return [HIPCC] + FLAGS[:3] + ["-c"] + FLAGS[3:] + extra + sf + ["-o", o + ".tmp", src]


def _link_sig(out):
    extra = VARIANTS[out]
    h = hashlib.sha1()
    for src in SOURCES:
        h.update(_sig(_compile_cmd(out, src, extra)).encode())
    return h.hexdigest()


def build_lib(force=False, verbose=False, jobs=None):
    """Build every stale variant: each source compiled to an object in parallel (objects newer than
    their source and the headers are kept), then one link per variant. Returns the product path."""
    os.makedirs(os.path.join(os.path.dirname(OUT), "obj"), exist_ok=True)
    jobs = jobs or max(1, min(16, os.cpu_count() or 1))
    hdr_t = max(os.path.getmtime(h) for h in HEADERS)
    todo, links = [], []
    for out, extra in VARIANTS.items():
        if not force and not stale(out):
            continue
        objs = []
        for src in SOURCES:
            o = _obj(out, src)
            objs.append(o)
            cmd = _compile_cmd(out, src, extra)
            if force or not _obj_fresh(o, src, hdr_t, _sig(cmd)):
                todo.append((cmd, o))
        links.append((out, objs))
    running = []
    while todo or running:
        while todo and len(running) < jobs:
            cmd, o = todo.pop(0)
            if verbose:
                print(" ".join(cmd))
            running.append((subprocess.Popen(cmd), o, cmd))
        p, o, cmd = running.pop(0)
        if p.wait() != 0:
            for q, _, _ in running:
                q.wait()
            raise subprocess.CalledProcessError(p.returncode, f"hipcc -> {o}")
        os.replace(o + ".tmp", o)
        with open(o + ".sig", "w") as f:
            f.write(_sig(cmd) + "\n")
    for out, objs in links:
        cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", out + ".tmp"] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        os.replace(out + ".tmp", out)
        with open(out + ".sig", "w") as f:
            f.write(_link_sig(out) + "\n")
    return OUT


if __name__ == "__main__":
    print(build_lib(force="--force" in sys.argv, verbose=True))
