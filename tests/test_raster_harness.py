"""tests/raster_harness.py pinned on the CPU: the bytes of every scene the rasterizer's tests build, that callers get arrays of
their own, the boundaries of the checks (on synthetic arrays) and the fields of `fake_cfg`.

The digests are sha256 over the bytes of means3D, scales, rotations, opacities, colors and the camera's view and projection
matrices.  They were recorded from the scene constructions that the test files held before the harness existed (up to eight
copies per scene, all in agreement); a digest that changes means a scene changed for every test that uses it."""
import hashlib

import numpy as np
import pytest
import torch

import raster_harness as rh

# scene(*key): every argument tuple that a test passes
SCENES = {
    (1, 40, 24, 1): "eef510bbbe916c745cad92e7714c6ff2d130f131d2f03f73213910fa388dea72",
    (1, 64, 48, 1): "dbbb8d41dc30aa05d6026edcf7a3d2e33e807e4fb42c4b5ee19be74269a9519f",
    (1, 64, 48, 2): "4394cfb08934b2538e14b1e70f4a16ef12dcc13a2fbbee82f0bcf13ff00557fa",
    (1, 64, 48, 3): "e79c1bd9662a264310811271c4ab3a371444441d71114658f939aaef25692c52",
    (1, 64, 48, 4): "6e5d1a16225cafab92ee75bbb60fd4a20b8da4e76935aa64166aeb4fb50f7640",
    (1, 64, 48, 6): "1fb4df9b1e1c37c529412360a57e0a769f9f1a32dcb674e3173563df6b0fb41c",
    (1, 64, 48, 8): "9869757706d942988a10939f3b7bc95cadac55da87bab845ce5f28e2a9ad640a",
    (64, 40, 24, 64): "dca32dc4f1d0f5c08c20e705443f76fe2c1f79e05bfd53bac2356780e9fc8467",
    (64, 128, 96, 64): "d3b2b60a2aae4f766688c701dbfd25a2208038c507a3d7b42944053ff7c54322",
    (64, 128, 96, 65): "73c18cba133c29df8a8611e8ce015d621472a736a86744d22a1238a46753220c",
    (64, 128, 96, 66): "c0b48c910c753206242b687647298f5a8420cac928c60894b33b93b3b319099f",
    (64, 128, 96, 67): "97ec2681130f7c7bb1f8495934cb7c3bb91014d001de2cc4f99d1caaa8ee8dc6",
    (64, 128, 96, 69): "7bdc1337b51b007d0b95d1cd82856bb665d5c6b3b8b6d1a9aa24a870dcf8bf33",
    (64, 128, 96, 71): "d8a87238430f292bc34c31ebf01172192ba4fe45c0a245ae286a1625a30536c3",
    (64, 128, 96, 77): "2f4ce7cc98f676a781f542ebd82d1a20f36cb0b946ce15d855fd83bf3ef4522f",
    (200, 64, 48, 0, 1.0, (0.005, 0.05)): "82477c487e0064d4a32d647b74470453aa9359f26d5920288c3673717117b2de",
    (200, 40, 24, 3, 1.0, (0.02, 0.12)): "7d3e5c0906e580802603f17ffb74a3d385e9567973110ff3ea0e3cdb2026ac88",
    (300, 40, 24, 7, 1.0, (0.01, 0.12)): "152ad13fd703150622d588cec3b8e5b05abe020f1a6158faa9c0b77d6d234799",
    (500, 65, 47, 4): "45a0aca2a7c94e588275728fe92685de616ccc601c01799084c0912e2dfc02b1",
    (2000, 128, 96, 7): "a3c543e0abdd939dc0db4380439e77fd660070694b2bb434c1970e0022faf8b5",
    (2000, 128, 96, 7, 1.0, (0.005, 0.05), (-1.5, -1.8, 0.9)): "b0cd29aa441dfb5dc1246f422ec32e140cf6f7507f0dec524f6ff385acc82729",
    (2000, 128, 96, 2003): "2e43d40d564bbf890e4020c39d6b7438054922d7bd13db8b6b4b38517f3fed99",
    (2000, 160, 120, 13): "bac7489ab33d76f51c42c3211e0e2405bff377dbd23137df4c3d848fb92754c6",
    (3000, 256, 256, 1, 1.0, (0.003, 0.04)): "185545132c3b1412d239507e18a03928643606c518a302325a58040c1399b58a",
    (3000, 256, 256, 21): "dd01fe43577aa90a90bca2dafdc182fcc49d547bcf757072b6fb4c6632fa024b",
    (3000, 256, 256, 41): "422497dd2589d9d2c642a5fbd605e0c289500fa52af588f0b5ef1f64cadb192a",
    (4000, 256, 256, 31): "37f9af38343cddcc89b3e79fcbf50e1b1d46ea6ffe6b1a1e2c34fd3765ac5a18",
    (4000, 256, 256, 4000): "ea68096f557f8fa1e65960864666b30996d296b24f1a542b6aeb500c89a2ea59",
    (4000, 256, 256, 4001): "6fa37b442ddc81c2d6dcb5853e84cb3b588f6227ee43d1091eb11e4c8d89e482",
    (4000, 256, 256, 4002): "4d90f7f1a21554fc59e280c590a5e398b74a1b3a3e12ca27143b28d7573cbc56",
    (4000, 256, 256, 4003): "6a8494e4b4ac554dcc1f9459698a552b94df0160c4d26173d3564c8935735078",
    (4000, 256, 256, 4005): "7ccdeaf5f0b7627174b7cd0b70c05f7300b988c2ff198227995b4c0d11de5fea",
    (4000, 256, 256, 4007): "13210528711e67bc5d39ca7715285913fc392f17c50eb5566f63c3ca5a6255b3",
    (4000, 256, 256, 4011): "3270d692efc792016f9eb74db2470c671413c443ee2f146e11f947a3e58fd569",
    (4000, 256, 256, 4013): "b7f38353db6c1b527f25709cee4c489bd21d9c868a1b56eba72a47b904634233",
    (5000, 257, 255, 4): "b91545b95f944a3901a98be6125493a0afe68dd25af848ec90b3be0d7b749863",
    (20000, 200, 120, 2, 1.2, (0.002, 0.03)): "c239d4903da9916fa4156f89aed6df312a3e529012b595307d6effde1c152d19",
    (20000, 320, 240, 9): "4819c200b87a87009e31868b20b218ee9b88b168a0d7cb4a315ec5f53597c443",
    (30000, 800, 600, 9): "caa5e43853770f62d380e3dcbebdf3cca63f9b4c97552b212835714e0b92a86f",
    (30000, 800, 800, 21): "cd39e8670abab72678e9f78f675612a24a7b4f3442c32d32484b68c5fa5c53cf",
    (30000, 800, 800, 30000): "345fe7b44ef5c3327bc25571c14b1de850306708a054efc0cc92996230a610a7",
    (30000, 800, 800, 30001): "10311e9747a05eebd636eefc809126dc10380913824c1be2949cb30ca1367000",
    (30000, 800, 800, 30002): "429329e5f603da94ac21616c145f70367ef32295effcbbf698bbcd6eda9b6189",
    (30000, 800, 800, 30003): "64ac02a09acfee2856c2df9eba25d67d4a4f29cb5258b01bc8ffcd86ff13c592",
    (30000, 800, 800, 30005): "93470ca752f21ef7e6e0eb8eb83ead83629446299eeed65acd23ff65e2d6f175",
    (30000, 800, 800, 30007): "1fec8d048bffa1e1ebeba925dd03b45bc23c2a129051a66623ba61be427a6fda",
    (30000, 800, 800, 30011): "57aa202f3b5583dcbc005a3b331774fc72a8b91a1af903024ac95bcf7450a2e3",
    (30000, 800, 800, 30013): "b053a89f09e26c795c2ffea21d7ad5f35a1055f366565ccb1a355af949d1911e",
    (200000, 1920, 1080, 31): "6c3248bf6d45ba24d64d1cf8f9aa174c4555b14cd156addf0f950f24739e1557",
    (200000, 1920, 1080, 200000): "c840e54fedc0bfc00f80835f304330f65443ea2ad7df1dc3b315add54320bbf5",
    (200000, 1920, 1080, 200001): "73475f15ea5ada79c6f3848d6c6f7276f2be9ceecfb837aa4f2aeb1796cbbb5a",
    (200000, 1920, 1080, 200002): "6b8a6bb41223341270f7737e78679aaa567fdedb06ce86ca64f990f3a494e1a8",
    (200000, 1920, 1080, 200003): "60fd8be1bf9dd3e04a5cb1fdb11100b214e9a7913e93a5745de074d383509ab0",
    (200000, 1920, 1080, 200005): "9741501281f33bcbf68747d179c797526597724a61cf935777967cc347e16c65",
    (200000, 1920, 1080, 200007): "5d18a82f453e348ed485d3db380dee913b0f366b0994bc2fbd6bcee4eb691131",
}
STACKS = {      # stack_scene(*key)
    ("saturated", 64, 48): "c875fa188d47cd9468f0f9f08f2bff6710e89c039c83b735e30ded8769f3e08e",
    ("long", 64, 48): "55253ae8f253666adfa03d0a04862cb79377e5611edcfaac70b17a747b8df55b",
    ("saturated", 16, 16): "d80ef79adde863cd2d4faf824f86912b8e3aafa373d34b238ee27ed94995e51e",
    ("long", 16, 16): "285bdff12de42009b689b791ba33467d2bee2e4d73fd9e4099efe0c2822f703e",
    ("saturated", 32, 16): "fe0b363d40254300f829d29923c7d5cc0b63b10c46d0a3c1693ca22077b582b9",
    ("long", 24, 16): "106c0e2826aaa07cfcbffbbafe358ddc2e30673a197ba3d4dcc19211166ca12c",
}
NAMED = {       # named_scene(key)
    "ragged": "7d3e5c0906e580802603f17ffb74a3d385e9567973110ff3ea0e3cdb2026ac88",
    "single": "dbbb8d41dc30aa05d6026edcf7a3d2e33e807e4fb42c4b5ee19be74269a9519f",
    "long": "285bdff12de42009b689b791ba33467d2bee2e4d73fd9e4099efe0c2822f703e",
    "saturated": "d80ef79adde863cd2d4faf824f86912b8e3aafa373d34b238ee27ed94995e51e",
}


def digest(cam, g):
    h = hashlib.sha256()
    for a in (g["means3D"], g["scales"], g["rotations"], g["opacities"], g["colors"], cam.world_view_transform,
              cam.full_proj_transform):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def test_scene_digests():
    assert {k: digest(*rh.scene(*k)) for k in SCENES} == SCENES


def test_stack_and_named_scene_digests():
    assert {k: digest(*rh.stack_scene(*k)) for k in STACKS} == STACKS
    assert {k: digest(*rh.named_scene(k)) for k in NAMED} == NAMED


@pytest.mark.parametrize("make, want", [(lambda: rh.scene(2000, 128, 96, 7), SCENES[(2000, 128, 96, 7)]),
                                        (lambda: rh.stack_scene("long", 16, 16), STACKS[("long", 16, 16)]),
                                        (lambda: rh.named_scene("ragged"), NAMED["ragged"])], ids=["scene", "stack", "named"])
def test_every_caller_gets_arrays_of_its_own(make, want):
    (_, a), (_, b) = make(), make()
    for k in a:
        assert not np.shares_memory(a[k], b[k]), k
    before = {k: v.copy() for k, v in b.items()}
    for k in a:
        a[k][:] = 7.0           # the in-place edit some tests make (g["opacities"][:] = ...)
    for k in b:
        assert np.array_equal(b[k], before[k]), k
    assert digest(*make()) == want


# ---- check_map ------------------------------------------------------------------------------------------------------------------
N = 100_000


def _off(n_out, delta, base=0.0):
    """A reference of N values with maximum 1 and an input that is `base` off everywhere and `delta` off on n_out values."""
    b = np.zeros(N, np.float32)
    b[0] = 1.0
    a = b + np.float32(base)
    a[1:1 + n_out] = b[1:1 + n_out] + np.float32(delta)
    return a, b


@pytest.mark.parametrize("cap", [1.0, 0.5])
def test_check_map_boundaries(cap):
    allowed = int(round(1e-4 * cap * N))          # 10 and 5 values beyond 2e-5
    rh.check_map(*_off(allowed, 3e-5), "at the allowed share", cap=cap)
    with pytest.raises(AssertionError):
        rh.check_map(*_off(allowed + 1, 3e-5), "one more", cap=cap)
    rh.check_map(*_off(0, 0.0, base=0.99e-5 * cap), "rmse just below", cap=cap)      # nothing beyond 2e-5: only the RMSE speaks
    with pytest.raises(AssertionError):
        rh.check_map(*_off(0, 0.0, base=1.01e-5 * cap), "rmse just above", cap=cap)


def test_check_map_takes_tensors_and_keeps_its_scale_floor():
    a, b = _off(10, 3e-5)
    rh.check_map(torch.tensor(a).reshape(1, 250, 400), b.reshape(1, 250, 400), "a tensor against an array")
    zero = np.zeros(N, np.float32)
    rh.check_map(zero, zero, "all zero")          # the scale is max(|b|, 1e-12)
    with pytest.raises(AssertionError):
        rh.check_map(zero + np.float32(1e-3), zero, "non-zero against all zero")


# ---- check_grad -----------------------------------------------------------------------------------------------------------------
def _grad_off(n_out, delta, shape=(1000, 5)):
    b = np.zeros(shape, np.float32)
    b.reshape(-1)[0] = -1.0
    a = b.copy()
    a.reshape(-1)[1:1 + n_out] += np.float32(delta)
    return a, b


@pytest.mark.parametrize("allow_frac, allowed", [(2e-3, 10), (1e-3, 5)])
def test_check_grad_boundaries(allow_frac, allowed):
    rh.check_grad(*_grad_off(allowed, 3e-4), "at the allowed share", allow_frac=allow_frac)
    with pytest.raises(AssertionError):
        rh.check_grad(*_grad_off(allowed + 1, 3e-4), "one more", allow_frac=allow_frac)
    rh.check_grad(*_grad_off(5000, 1.9e-4), "every entry just inside 2e-4 of the maximum", allow_frac=allow_frac)
    a, b = _grad_off(allowed + 1, 3e-4)
    rh.check_grad(torch.tensor(a), b, "a wider tol", allow_frac=allow_frac, tol=4e-4)


def test_check_grad_defaults_and_scale_floor():
    rh.check_grad(*_grad_off(10, 3e-4), "defaults: a 2e-3 share beyond 2e-4")
    with pytest.raises(AssertionError):
        rh.check_grad(*_grad_off(11, 3e-4), "defaults, one more")
    a, b = _grad_off(2, 3e-4, shape=(1000,))        # a [P] tensor is one column
    rh.check_grad(torch.tensor(a), b, "one column")
    zero = np.zeros((1000, 5), np.float32)
    rh.check_grad(zero, zero, "all zero")         # the scale is max(1e-6, |b|)
    with pytest.raises(AssertionError):
        rh.check_grad(zero + np.float32(1e-3), zero, "non-zero against all zero")
    rh.check_grad(zero + np.float32(1e-10), zero, "1e-10 against all zero: 1e-4 of the floor")


# ---- check_image ----------------------------------------------------------------------------------------------------------------
def _image_off(n_out, delta, base=0.0):
    a, b = _off(n_out, delta, base)
    return torch.tensor(a).reshape(1, 250, 400), torch.tensor(b).reshape(1, 250, 400)


def test_check_image_boundaries(capsys):
    rh.check_image(*_image_off(10, 3e-5), 1e-5, "at the allowed share")
    assert "[allowance] at the allowed share: rmse" in capsys.readouterr().out
    with pytest.raises(AssertionError):
        rh.check_image(*_image_off(11, 3e-5), 1e-5, "one more")
    rh.check_image(*_image_off(0, 0.0, base=0.99e-5), 1e-5, "rmse just below")
    with pytest.raises(AssertionError):
        rh.check_image(*_image_off(0, 0.0, base=1.01e-5), 1e-5, "rmse just above")
    rh.check_image(*_image_off(1, 1.0 / 255), 1e-4, "one alpha decision")
    with pytest.raises(AssertionError):
        rh.check_image(*_image_off(1, 1.0 / 255 + 2e-4), 1e-4, "more than one alpha decision")
    capsys.readouterr()
    rh.check_image(*_image_off(10, 3e-5), 1e-5)
    assert capsys.readouterr().out == ""          # unnamed: no line
    with pytest.raises(AssertionError):
        rh.check_image(*_image_off(11, 3e-5), 1e-5)


def test_close_counts_rows():
    b = torch.zeros(1000, 3)
    b[0, 0] = 1.0
    a = b.clone()
    a[1:3, 1] += 3e-4
    rh.close(a, b, "two rows of 1000 at 2e-3", allow_frac=2e-3)
    with pytest.raises(AssertionError):
        rh.close(a, b, "two rows of 1000 at 1e-3", allow_frac=1e-3)
    with pytest.raises(AssertionError):
        rh.close(a, b, "no allowance", allow_frac=0.0)
    rh.close(a, b, "the rows that agree", rows=torch.arange(1000) > 2, allow_frac=0.0)
    with pytest.raises(TypeError):
        rh.close(a, b, "the allowance is the caller's to state")


# ---- fake_cfg -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W, campos", [(16, 16, True), (16, 16, False), (40, 24, True)])
def test_fake_cfg_fields(H, W, campos):
    cfg = rh.fake_cfg(H=H, W=W, campos=campos)
    got = {name: getattr(cfg, name) for name, _ in cfg._fields_}
    assert got == dict(image_height=H, image_width=W, tanfovx=0.5, tanfovy=0.5, scale_modifier=1.0, prefiltered=0, debug=0,
                       viewmatrix=256, projmatrix=256, campos=256 if campos else None, bg=256)
    if (H, W, campos) == (16, 16, True):
        assert bytes(cfg) == bytes(rh.fake_cfg())
