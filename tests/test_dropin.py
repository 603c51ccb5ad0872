"""The drop-in layer: shim packages carry the reference's import names, and modules laid out like the
reference's own GaussianModel / render code import on top of them and get their hot-path names rebound."""
import importlib
import sys

import pytest


def test_shims_expose_reference_import_names():
    import contextgs_amd.dropin as dropin
    dropin.install(patch_reference_python=False)
    dgr = importlib.import_module("diff_gaussian_rasterization")
    assert hasattr(dgr, "GaussianRasterizationSettings") and hasattr(dgr, "GaussianRasterizer")
    fields = dgr.GaussianRasterizationSettings._fields
    assert fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix",
                      "projmatrix", "sh_degree", "campos", "prefiltered", "debug")      # gaussian_renderer/__init__.py:179-192
    ta = importlib.import_module("torchac")
    assert callable(ta.encode_float_cdf) and callable(ta.decode_float_cdf)
    em = importlib.import_module("compressai.entropy_models")
    assert callable(importlib.import_module("torch_scatter").scatter_max)              # scene/gaussian_model.py:24
    eb = em.EntropyBottleneck(channels=12)
    for m in ("forward", "quantize", "compress", "decompress", "update", "_get_medians"):
        assert hasattr(eb, m)


# A stand-in for the reference checkout's Python modules that the drop-in layer serves: their imports of the native wheels
# (answered by the shims) and of each other, and the names install() rebinds (the function bodies are irrelevant here).
# The import lines are those at the top of the reference's scene/gaussian_model.py, utils/encodings.py,
# utils/entropy_models.py and gaussian_renderer/__init__.py that name a shimmed package (compressai, plyfile, simple_knn,
# torch_scatter, torchac, diff_gaussian_rasterization) or another of these modules; imports of packages that are used as
# installed (torch, numpy, einops, the standard library) are left out, since the shims have no part in them.  The rebound
# names are the ones contextgs_amd/dropin/__init__.py lists.
_REFERENCE_LAYOUT = {
    "scene/__init__.py": "",
    "scene/gaussian_model.py": """
import compressai
from plyfile import PlyData, PlyElement
from simple_knn._C import distCUDA2
from torch_scatter import scatter_max
from compressai.entropy_models import EntropyBottleneck, GaussianConditional
from compressai.latent_codecs import LatentCodec, HyperLatentCodec
from utils.entropy_models import Entropy_bernoulli, Entropy_gaussian, Entropy_factorized
from utils.multi_level import torch_unique_with_indices
from utils.encodings import STE_binary, STE_multistep, Quantize_anchor, get_binary_vxl_size, encoder, decoder, \\
    encoder_gaussian, decoder_gaussian


def multi_scale_generating(*a, **k): raise NotImplementedError
def extract_context_feat(*a, **k): raise NotImplementedError
def find_divide_scale(*a, **k): raise NotImplementedError
def divide_levels(*a, **k): raise NotImplementedError
def mapping_to_orign(*a, **k): raise NotImplementedError
def index_of_level_L_in_orign(*a, **k): raise NotImplementedError


class GaussianModel:
    def training_statis(self, *a, **k): raise NotImplementedError
    def anchor_growing(self, *a, **k): raise NotImplementedError
    def adjust_anchor(self, *a, **k): raise NotImplementedError
    def prune_anchor(self, mask): raise NotImplementedError
    def cat_tensors_to_optimizer(self, d): raise NotImplementedError
    def conduct_encoding(self, p): raise NotImplementedError
    def conduct_decoding(self, p): raise NotImplementedError
    def estimate_final_bits(self): raise NotImplementedError
""",
    "utils/__init__.py": "",
    "utils/encodings.py": """
import torchac
use_clamp = True
class STE_binary: pass
class STE_multistep: pass
class Quantize_anchor: pass
def get_binary_vxl_size(*a, **k): raise NotImplementedError
def encoder(*a, **k): raise NotImplementedError
def decoder(*a, **k): raise NotImplementedError
def encoder_gaussian(*a, **k): raise NotImplementedError
def decoder_gaussian(*a, **k): raise NotImplementedError
""",
    "utils/entropy_models.py": """
from utils.encodings import use_clamp
class Entropy_gaussian: pass
class Entropy_gaussian_clamp: pass
class Entropy_bernoulli: pass
class Entropy_factorized: pass
class Low_bound: pass
class UniverseQuant: pass
""",
    "utils/multi_level.py": "def torch_unique_with_indices(*a, **k): raise NotImplementedError\n",
    "utils/loss_utils.py": "def l1_loss(*a, **k): raise NotImplementedError\ndef ssim(*a, **k): raise NotImplementedError\n",
    "gaussian_renderer/__init__.py": """
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
from scene.gaussian_model import GaussianModel, multi_scale_generating
from utils.encodings import STE_binary, STE_multistep
from utils.multi_level import torch_unique_with_indices
def generate_neural_gaussians(*a, **k): raise NotImplementedError
def render(*a, **k): raise NotImplementedError
def prefilter_voxel(*a, **k): raise NotImplementedError
""",
}


def test_reference_python_imports_on_top_of_the_shims(tmp_path):
    import contextgs_amd.dropin as dropin
    for rel, text in _REFERENCE_LAYOUT.items():
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text(text)
    sys.path.insert(0, str(tmp_path))
    try:
        dropin.install(patch_reference_python=False)
        gm = importlib.import_module("scene.gaussian_model")
        importlib.import_module("gaussian_renderer")
        patched = dropin.install()
        assert "scene.gaussian_model.multi_scale_generating" in patched
        assert "scene.gaussian_model.GaussianModel.training_statis" in patched
        assert "scene.gaussian_model.GaussianModel.anchor_growing" in patched
        assert "utils.loss_utils.ssim" in patched
        from contextgs_amd import context_model
        assert gm.multi_scale_generating is context_model.multi_scale_generating
        assert gm.EntropyBottleneck.__module__ == "contextgs_amd.entropy_bottleneck"
    finally:
        sys.path.remove(str(tmp_path))
        for k in [k for k in sys.modules if k.split(".")[0] in ("scene", "utils", "gaussian_renderer", "arguments")]:
            del sys.modules[k]


def test_install_repoints_a_loaded_script_without_importing_train():
    """train.py binds render / l1_loss / ssim by name (train.py:36-37): install() re-points modules that already hold
    them (`train`, `__main__`) and never imports `train` itself (that would run the script's top level twice)."""
    import types
    import contextgs_amd.dropin as dropin
    from contextgs_amd import loss_utils, renderer
    sys.modules.pop("train", None)
    dropin.install()
    assert "train" not in sys.modules                      # not imported as a side effect
    fake = types.ModuleType("train")
    def ref_fn(module):                                    # stands for a function the reference's module defined
        f = lambda *a, **k: None
        f.__module__ = module
        return f
    fake.render, fake.prefilter_voxel = ref_fn("gaussian_renderer"), ref_fn("gaussian_renderer")
    fake.l1_loss, fake.ssim = ref_fn("utils.loss_utils"), ref_fn("utils.loss_utils")
    fake.unrelated = 1
    own_render = ref_fn("my_viewer")                       # an unrelated script's own `render` must survive install()
    other = types.ModuleType("__main__")
    other.render = own_render
    real_main = sys.modules["__main__"]
    sys.modules["__main__"] = other
    sys.modules["train"] = fake
    try:
        patched = dropin.install()
        assert fake.render is renderer.render and fake.prefilter_voxel is renderer.prefilter_voxel
        assert fake.l1_loss is loss_utils.l1_loss and fake.ssim is loss_utils.ssim and fake.unrelated == 1
        assert "train.render" in patched and "train.ssim" in patched
        assert other.render is own_render and "__main__.render" not in patched
    finally:
        sys.modules["__main__"] = real_main
        del sys.modules["train"]
        for k in [k for k in sys.modules if k.split(".")[0] in ("scene", "utils", "gaussian_renderer", "arguments")]:
            del sys.modules[k]


def test_latent_codec_checkpoint_must_carry_the_density_parameters():
    import torch
    from contextgs_amd.codec_driver import _load_latent_codec
    from contextgs_amd.entropy_bottleneck import EntropyBottleneck
    src = EntropyBottleneck(12)
    with torch.no_grad():
        for p in src.parameters():
            p.add_(torch.randn_like(p) * 0.1)
    sd = src.state_dict()
    dst = EntropyBottleneck(12)
    _load_latent_codec(dst, sd)
    assert all(torch.equal(a, b) for a, b in zip(src.parameters(), dst.parameters()))
    # names of older compressai releases are remapped
    legacy = {}
    for k, v in sd.items():
        head, _, idx = k.partition(".")
        legacy["_" + {"matrices": "matrix", "biases": "bias", "factors": "factor"}[head] + idx if head in ("matrices", "biases", "factors") else k] = v
    dst = EntropyBottleneck(12)
    _load_latent_codec(dst, legacy)
    assert all(torch.equal(a, b) for a, b in zip(src.parameters(), dst.parameters()))
    # a checkpoint without them is an error, not a silently random prior
    with pytest.raises(RuntimeError, match="density parameters"):
        _load_latent_codec(EntropyBottleneck(12), {k: v for k, v in sd.items() if not k.startswith("factors")})
