"""The streaming layer is split over sibling modules; ``bvcodec.streaming`` still offers every name it offered as one file, and the host
arithmetic imports without torch.  No device."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("StreamingEncoder", "VocoderStream", "StreamingDecoder", "StreamingCodec", "StreamResampler",
         "CONTEXT_FRAMES", "join_plan", "finish_plan", "generator_reach", "repair_plan", "client_hop", "client_finish_plan",
         "PCM_FORMATS", "PCM_DTYPES", "PCM_DELAYED", "pcm_s16_to_f32", "pcm_f32_to_s16", "resampler_count", "resampler_lag")
HOMES = {"stream_plans": NAMES[5:12], "resampling": NAMES[4:5] + NAMES[12:], "stream_chunked": NAMES[:3]}


def test_every_name_is_importable_from_streaming():
    import importlib
    streaming = importlib.import_module("bvcodec.streaming")
    for name in NAMES:
        assert hasattr(streaming, name), name
    assert sorted(n for names in HOMES.values() for n in names) == sorted(set(NAMES) - {"StreamingCodec"})
    for module, names in HOMES.items():                         # ... and is the very object of the module that holds it
        home = importlib.import_module("bvcodec." + module)
        for name in names:
            assert getattr(streaming, name) is getattr(home, name), (module, name)
    assert streaming.StreamingCodec.__module__ == "bvcodec.streaming"


def test_stream_plans_imports_without_torch():
    code = ("import sys; sys.path.insert(0, %r); import bvcodec.stream_plans as p; "
            "assert p.join_plan(0, 441) == (0, 0, 1) and p.client_hop(320, 16000) == 441; "
            "bad = [m for m in sys.modules if m == 'torch' or m.startswith('torch.') or m.endswith('._abi')]; "
            "assert not bad, bad") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
