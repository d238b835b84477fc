"""The facade is split over sibling modules; ``bvcodec.model`` still offers every name it offered as one file, the closed-loop argument
checks import without torch, and the Python statement of the front-end's frame count gives the values ``bvc_num_frames`` gives
(``tests/test_gpu_facade_args.py`` holds it against the library itself).  No device."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOMES = {"model": ("BVRNNCodecModel", "SCALING", "default_config", "default_chkpt_bvrnn", "default_chkpt_vocoder"),
         "coder": ("BVRNN", "BigVGAN"), "vbr_args": ("cap_q8", "_check_ladder"), "engine": ("_Engine",)}


def test_every_name_is_importable_from_model():
    import importlib
    model = importlib.import_module("bvcodec.model")
    for module, names in HOMES.items():                         # ... and is the very object of the module that holds it
        home = importlib.import_module("bvcodec." + module)
        for name in names:
            assert getattr(model, name) is getattr(home, name), (module, name)
            if callable(getattr(model, name)):                  # defined there, not imported into it
                assert getattr(model, name).__module__ == "bvcodec." + module, (module, name)


def test_vbr_args_imports_without_torch():
    code = ("import sys; sys.path.insert(0, %r); import bvcodec.vbr_args as v; "
            "bad = [m for m in sys.modules if m == 'torch' or m.startswith('torch.') or m.endswith('._abi')]; "
            "assert not bad, bad; "
            "assert v.cap_q8({'hopsize': 256, 'fs': 22050}, [8, 16], 0, 8) == (0, 2048)") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_frame_count(conf_var):
    """bvc_num_frames with winsize 1024, hopsize 256, mel_pad_left 256: nothing while the right reflect padding (512 samples) is not
    shorter than the signal, then (L - 256) // 256 + 1."""
    from bvcodec.config import num_frames
    assert (conf_var["winsize"], conf_var["hopsize"], conf_var["mel_pad_left"]) == (1024, 256, 256)
    want = {0: 0, 256: 0, 512: 0, 513: 2, 767: 2, 768: 3, 1024: 4, 1025: 4}
    assert {L: num_frames(conf_var, L) for L in want} == want
