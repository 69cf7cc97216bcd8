"""Float32 NCHW input (the reference's normalised ``Data`` batches) without a GPU: argument validation of
gv_patchify_nchw / gv_patchify_nchw_f32, the float batch mode of TileFolder, and the driver's refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(**kw):
    from gipvit import _lib
    a = _lib.gv_patchify_nchw_args()
    a.images, a.patches = 256, 256
    a.n_img, a.n_tiles, a.img_h, a.img_w = 2, 2, 256, 256
    a.stride_n, a.stride_c, a.stride_h = 3 * 256 * 256, 256 * 256, 256
    a.n_win, a.crop = 1, 224
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("name", ["gv_patchify_nchw", "gv_patchify_nchw_f32"])
def test_patchify_nchw_argument_validation(name):
    from gipvit import _lib
    fn = getattr(_lib.lib, name)

    def rc(a):
        return fn(ctypes.byref(a), None), _lib.lib.gv_last_error().decode()

    code, msg = rc(_args(images=None))
    assert code == -3 and "null" in msg and name in msg
    code, msg = rc(_args(patches=None))
    assert code == -3 and "null" in msg
    code, msg = rc(_args(crop=100))
    assert code == -1 and "crop=100" in msg and "multiple of 16" in msg
    a = _args(); a.win_y[0], a.win_x[0] = 16, 40           # 40 + 224 > 256
    code, msg = rc(a)
    assert code == -1 and "window 0 (16,40)+224" in msg and "256x256" in msg
    code, msg = rc(_args(n_img=3))
    assert code == -1 and "n_img (3)" in msg and "n_tiles (2)" in msg
    code, msg = rc(_args(n_win=17, n_img=34))
    assert code == -1 and "n_win" in msg
    code, msg = rc(_args(patches=258))                      # patch rows are written with 16-byte stores
    assert code == -2 and "16-byte" in msg


def test_patchify_nchw_symbols_in_both_builds():
    """Both library builds export the two entry points (the f16 build is loaded in a process of its own)."""
    import subprocess
    pkg = os.path.join(ROOT, "gipmed-project-self-supervised-vit_amd")
    for lib in ("libgipvit_hip.so", "libgipvit_hip_f16.so"):
        code = f"import ctypes; l = ctypes.CDLL({os.path.join(pkg, lib)!r}); l.gv_patchify_nchw; l.gv_patchify_nchw_f32"
        subprocess.run([sys.executable, "-c", code], check=True)


def test_input_form_rejects_other_types_without_gpu():
    from gipvit.engine import input_form
    assert input_form(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), 2, (8, 8)) == "u8"
    assert input_form(torch.zeros(2, 3, 8, 8), 2, (8, 8)) == "f32"
    for bad in (torch.zeros(2, 8, 8, 3), torch.zeros(2, 3, 8, 8, dtype=torch.float16), torch.zeros(2, 3, 8, 8, dtype=torch.float64),
                torch.zeros(2, 3, 8, 8).to(memory_format=torch.channels_last), torch.zeros(3, 8, 8)):
        with pytest.raises(TypeError, match=r"uint8 NHWC tiles \[n, H, W, 3\] or float32 NCHW \[n, 3, H, W\]"):
            input_form(bad, 2, (8, 8))
    with pytest.raises(ValueError, match="shape"):
        input_form(torch.zeros(3, 3, 8, 8), 2, (8, 8))
    with pytest.raises(ValueError, match="boxes="):
        input_form(torch.zeros(2, 3, 8, 8), 2, (8, 8), (("fill", None), ("boxes", (1, 2))))
    assert input_form(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), 2, (8, 8), (("boxes", (1, 2)),)) == "u8"


def _tiles(root, n_slides=2, n=3, t=32):
    from gipvit import data as D
    rng = np.random.default_rng(0)
    for s in range(n_slides):
        os.makedirs(root / f"slide{s}", exist_ok=True)
        for i in range(n):
            D.write_tile_file(str(root / f"slide{s}" / f"tile_{i}.data"), rng.integers(0, 256, (t, t, 3), dtype=np.uint8))
    (root / "labels.csv").write_text("slide,label,fold\n" + "".join(f"slide{s},{s % 2},{1 + s % 2}\n" for s in range(n_slides)))


MEAN, STD = np.array([0.8998, 0.8253, 0.9357], np.float32), np.array([0.1125, 0.1751, 0.0787], np.float32)


def float_hook(tile):
    """ToTensor + Normalize, as the reference's hooks end (transformations.py:124-128): uint8 HWC -> float [3, H, W]."""
    x = torch.from_numpy(np.array(tile)).permute(2, 0, 1).float() / 255.0
    return (x - torch.from_numpy(MEAN)[:, None, None]) / torch.from_numpy(STD)[:, None, None]


def test_tilefolder_float_hook_batches(tmp_path):
    from gipvit import data as D
    _tiles(tmp_path)
    src = D.TileFolder(str(tmp_path), batch=2, transform=float_hook, seed=0, tile_size=32, n_tiles=3)
    assert src.batch_format == "f32_nchw"
    batches = list(src)
    assert len(batches) == 3
    files = {p: D.read_tile_file(p) for s in src.slides for p in s[1]}
    for b in batches:
        assert b["Data"].dtype == torch.float32 and b["Data"].shape == (2, 3, 32, 32) and b["Target"].shape == (2, 1)
        for x in b["Data"]:         # every image is the hook's output of one of the files, exactly
            assert any(torch.equal(x, float_hook(t)) for t in files.values())
    # the numpy form of the same hook, and the u8 forms, are told apart
    assert D.TileFolder(str(tmp_path), 2, lambda t: float_hook(t).numpy(), tile_size=32, n_tiles=3).batch_format == "f32_nchw"
    assert D.TileFolder(str(tmp_path), 2, lambda t: t[::-1].copy(), tile_size=32, n_tiles=3).batch_format == "u8_nhwc"
    assert D.TileFolder(str(tmp_path), 2, None, tile_size=32, n_tiles=3).batch_format == "u8_nhwc"
    # a float HWC image is neither accepted form
    bad = D.TileFolder(str(tmp_path), 2, lambda t: float_hook(t).permute(1, 2, 0), tile_size=32, n_tiles=3)
    with pytest.raises(TypeError, match=r"float32 \(32, 32, 3\).*uint8 \[32, 32, 3\].*float \[3, 32, 32\]"):
        bad.batch_format
    # a float-mode source refuses a uint8 staging buffer
    with pytest.raises(TypeError, match="f32_nchw"):
        src.fill(np.empty((2, 32, 32, 3), np.uint8), np.empty((2, 1), np.int64))


def test_train_refuses_u8_only_features_with_float_hook(tmp_path, monkeypatch):
    """The refusals fire before any GPU work (this machine may have none: the CUDA check comes after them)."""
    sys.path.insert(0, ROOT)
    import train
    _tiles(tmp_path, t=64)
    base = ["--model", "vit_tiny_patch16_224", "--dataset", f"tiles:{tmp_path}", "--tile-size", "64", "-b", "2", "--output", str(tmp_path / "out")]
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("GPU check reached")))
    with pytest.raises(SystemExit, match="--random-crops: the transform hook returns float32"):
        train.main(base + ["--dino", "--random-crops", "--out-dim", "1024"], transform=float_hook)
    with pytest.raises(SystemExit, match="--view-augment"):
        train.main(base + ["--dino", "--view-augment", "--out-dim", "1024"], transform=float_hook)
    with pytest.raises(SystemExit, match="--transform_type pcbnfrsc"):
        train.main(base + ["--transform_type", "pcbnfrsc"], transform=float_hook)
    with pytest.raises(SystemExit, match="tiles read from disk"):
        train.main(["--model", "vit_tiny_patch16_224", "--dataset", "synthetic"], transform=float_hook)
    with pytest.raises(TypeError, match="transform hook returned"):
        train.main(base, transform=lambda t: t.astype(np.float32))
    # a u8 hook with --random-crops is not refused here: it gets as far as the GPU check
    with pytest.raises(AssertionError, match="GPU check reached"):
        train.main(base + ["--dino", "--random-crops", "--out-dim", "1024"], transform=lambda t: t.copy())
