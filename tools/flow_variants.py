"""Builds variant libraries of the persistent recurrence (k_flow.hip, which holds the kernel and includes its device code from
k_flow_handoff.h / k_flow_layers.h / k_flow_gru.h, with extra -D switches) next to the product library, and
times them against each other on the GPU box.

    python tools/flow_variants.py build base: depth2:-DBVC_GRU_DEPTH=2 "g2diag:-DBVC_CHAIN_G=2 -DBVC_FLOW_DIAG=1"     (here: cross-compiles)
    python tools/flow_variants.py run [--seconds 5] [--batch 64] [--reps 5] [--diag] name...                (on the GPU box)

Every variant runs in its own process (BVC_LIB selects the library); codes / mel of every variant are compared with the first one.
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bernoulli-var-speech-codec_amd", "csrc")
VDIR = os.path.join(CSRC, "variants")


def build(specs):
    sys.path.insert(0, ROOT)
    from bvcodec import build as b
    b.build(verbose=False)                     # the other objects
    os.makedirs(VDIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    procs = []
    for spec in specs:
        name, _, defs = spec.partition(":")
        o = os.path.join(VDIR, f"k_flow_{name}.o")
        cmd = [hipcc] + b.FLAGS + defs.split() + ["-c", os.path.join(CSRC, "k_flow.hip"), "-o", o]
        procs.append((name, o, subprocess.Popen(cmd)))
    for name, o, p in procs:
        if p.wait():
            raise SystemExit(f"variant {name}: compile failed")
        objs = [os.path.join(CSRC, f.replace(".hip", ".o")) for f in b.SOURCES if f != "k_flow.hip"] + [o]
        lib = os.path.join(VDIR, f"libbvcodec_{name}.so")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs)
        print("built", lib)


CHILD = r'''
import ctypes, hashlib, json, os, sys, tempfile, time
import torch
sys.path.insert(0, ROOT)
from bvcodec import BVRNNCodecModel, _abi, config, synth
secs, batch, reps, diag = SECS, BATCH, REPS, DIAG
conf = config.load_config(config.DEFAULT_CONFIG)
d = tempfile.mkdtemp()
p1, p2 = synth.write_checkpoints(conf, d, seed=1234)
model = BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2).to("cuda:0")
L = int(22050 * secs)
x = synth.synthetic_speech(batch, L, seed=0, kind="noise").cuda()
lib = _abi.load()
for _ in range(2):
    codes = model.encode(x, 3000); wav = model.decode(codes, L)
torch.cuda.synchronize()
def timeit(fn):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]
res = {}
mean, mn, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32()
_abi.check(lib.bvc_probe_begin(1, 1, 4096))
for _ in range(reps):
    codes = model.encode(x, 3000); wav = model.decode(codes, L)
_abi.check(lib.bvc_probe_end(ctypes.byref(mean), ctypes.byref(mn), ctypes.byref(n)))
res["flow_mean_us"] = round(mean.value, 1); res["flow_min_us"] = round(mn.value, 1)
res["encode_ms"], _ = timeit(lambda: model.encode(x, 3000))
res["decode_ms"], _ = timeit(lambda: model.decode(codes, L))
res["step_ms"] = round(res["encode_ms"] + res["decode_ms"], 3)
model.check_status()
res["codes_sha"] = hashlib.sha1(codes.cpu().numpy().tobytes()).hexdigest()[:12]
res["wav_sha"] = hashlib.sha1(wav.cpu().numpy().tobytes()).hexdigest()[:12]
if diag:
    def span(a, b, lo, hi):
        _abi.check(lib.bvc_kprobe_read_span(a, b, lo, hi, ctypes.byref(mean), ctypes.byref(mn), ctypes.byref(n)))
        return round(mean.value, 2)
    names = ["enc0", "enc1", "enc2", "pz0", "pz1", "pz2", "dec0", "dec1", "dec2", "dec3", "px0", "px1", "px2", "gru"]
    _abi.check(lib.bvc_kprobe_enable(1))
    for enc in (True, False):
        if enc: codes = model.encode(x, 3000)
        else: model.decode(codes, L)
        nm = names if enc else names[6:]
        rows = []
        for i, k in enumerate(nm):
            rows.append((k, span(0, 1, i, i + 1), span(0, 2, i, i + 1), span(2, 3, i, i + 1), span(3, 4, i, i + 1), span(4, 1, i, i + 1), span(0, 5, i, i + 1)))
        res["diag_encode" if enc else "diag_decode"] = rows
    _abi.check(lib.bvc_kprobe_enable(0))
print("RESULT " + json.dumps(res))
'''


def run(args):
    secs, batch, reps, diag = 5.0, 64, 5, False
    names = []
    it = iter(args)
    for a in it:
        if a == "--seconds": secs = float(next(it))
        elif a == "--batch": batch = int(next(it))
        elif a == "--reps": reps = int(next(it))
        elif a == "--diag": diag = True
        else: names.append(a)
    first = None
    for name in names:
        lib = os.path.join(VDIR, f"libbvcodec_{name}.so") if name != "product" else os.path.join(CSRC, "libbvcodec_hip.so")
        env = dict(os.environ, BVC_LIB=lib)
        src = (CHILD.replace("ROOT", repr(ROOT)).replace("SECS", repr(secs)).replace("BATCH", repr(batch))
               .replace("REPS", repr(reps)).replace("DIAG", repr(diag)))
        p = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode or not line:
            print(f"{name}: FAILED rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}", flush=True)
            continue
        r = json.loads(line[0][7:])
        if first is None:
            first = r
        same = r["codes_sha"] == first["codes_sha"] and r["wav_sha"] == first["wav_sha"]
        print(f"{name:14s} step {r['step_ms']:7.3f} ms  encode {r['encode_ms']:7.3f}  decode {r['decode_ms']:7.3f}  flow launch mean {r['flow_mean_us']:9.1f} us"
              f"  outputs {'identical' if same else 'DIFFER'} ({r['codes_sha']})", flush=True)
        for key in ("diag_encode", "diag_decode"):
            if key in r:
                print(f"  {key}: layer  entry->published | entry->flags | flags->products | products->barrier | barrier->published | entry->left")
                tot = 0.0
                for row in r[key]:
                    print("    %-5s %6.2f | %6.2f | %6.2f | %6.2f | %6.2f | %6.2f" % tuple(row))
                    tot += row[1]
                print(f"    sum entry->published {tot:.1f} us per frame")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build(sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "run":
        run(sys.argv[2:])
    else:
        print(__doc__)
