"""Multi-code GAN inversion (mGANprior) on the CPU: the test-side restatement of the demo's loop (tests/mgan_inv_util.py, on the
oracle's layer functions) reproduces tests/golden/mgan_inversion.npz (made from the reference's own modules by
tests/golden/make_mgan_inversion_golden.py); the layer names, their aliases and the refusals; invert's argument checks that
need no device; the command's new arguments and its unchanged CSV columns."""
import pytest
import torch

from tests.golden_util import load
from tests.mgan_inv_util import CASES, IDS, fixture_case, oracle_invert_multi
from tests.test_inversion_cpu import REF_COLUMNS


@pytest.mark.parametrize("arch,distance,layer", CASES, ids=IDS)
def test_restatement_reproduces_reference_fixture(arch, distance, layer):
    """the bounds test_inversion_cpu.test_restatement_reproduces_reference_fixture holds the single-code loop to; alpha (steps
    of at most 1e-3) to 1e-7"""
    g = load("mgan_inversion")
    c = fixture_case(g, arch, distance, layer)
    res = oracle_invert_multi(c["params"], arch, c["gumbel"], c["inv_ref"], c["mask"], c["latent0"][None], c["noise"][:, None],
                              c["S"], distance, layer)
    t = lambda k: torch.from_numpy(g[c["pre"] + k])
    for k, (loss, gz, ga, lat, al) in enumerate(res):
        assert torch.allclose(loss, t(f"s{k}/loss"), rtol=0, atol=1e-5), k
        assert torch.allclose(gz[0], t(f"s{k}/grad"), rtol=1e-4, atol=1e-6), k
        assert torch.allclose(ga[0], t(f"s{k}/dalpha"), rtol=1e-4, atol=1e-6), k
        assert torch.allclose(lat[0], t(f"s{k}/latent"), rtol=0, atol=1e-5), k
        assert torch.allclose(al[0], t(f"s{k}/alpha"), rtol=0, atol=1e-7), k


def test_fixture_gradients_are_away_from_zero():
    """what the generator script asserted: from step 1 on no gradient component is within 1e-4 of the largest (an early Adam
    step is about lr sign(g))"""
    g = load("mgan_inversion")
    for arch, distance, layer in CASES:
        c = fixture_case(g, arch, distance, layer)
        for k in range(1, c["S"]):
            for name in ("grad", "dalpha"):
                x = torch.from_numpy(g[c["pre"] + f"s{k}/{name}"]).abs()
                assert float(x.min() / x.max()) > 1e-4, (arch, layer, k, name)


def _tiny_G(arch):
    from dusty_gan_amd.models import dusty
    from dusty_gan_amd.models.gans.dcgan_eqlr import Generator
    heads = {"none": {"depth": 1}, "dusty2": {"depth": 1, "confidence": 2}}[arch]
    bb = Generator(8, heads, 4, 16, (32, 64), ring=True)
    return bb if arch == "none" else dusty.DUSty2(bb, tau=1, drop_const=-1)


def test_layer_names_aliases_and_refusals():
    from dusty_gan_amd.inversion import composition_layers, parse_composition_layer
    shapes = [(16, 2, 4), (16, 4, 8), (8, 8, 16), (4, 16, 32)]
    bare, wrapped = composition_layers(_tiny_G("none")), composition_layers(_tiny_G("dusty2"))
    assert list(bare) == ["0", "0.1", "1", "1.2", "2", "2.2", "3", "3.2"]
    assert list(wrapped) == ["backbone." + k for k in bare]
    for l in range(4):
        alias = f"{l}.{1 if l == 0 else 2}"
        for name in (str(l), alias):
            assert bare[name] == shapes[l] and wrapped["backbone." + name] == shapes[l]
            assert parse_composition_layer(name) == l and parse_composition_layer("backbone." + name) == l
            assert parse_composition_layer("backbone." + name, wrapped=True) == l
        assert parse_composition_layer(l) == l
    # the fixture's layer names are among the accepted ones
    g = load("mgan_inversion")
    for arch, distance, layer in CASES:
        assert parse_composition_layer(fixture_case(g, arch, distance, layer)["name"], wrapped=arch != "none") == layer
    # any other inner module: a Pad's output, a conv's pre-activation, the Head's inside, the Head, an index out of range
    for name in ("1.0", "1.1", "0.0", "backbone.2.0", "backbone.3.1", "4", "backbone.4", "4.heads.depth.1", "backbone.4.heads.confidence",
                 "backbone", "", 4, -1):
        with pytest.raises(NotImplementedError) as e:
            parse_composition_layer(name)
        assert "backbone.0" in str(e.value) and '"<blk>.2"' in str(e.value), name
    with pytest.raises(NotImplementedError):
        parse_composition_layer("backbone.2", wrapped=False)   # the bare generator has no such module


def test_argument_errors_need_no_device():
    from dusty_gan_amd.inversion import check_multi_code, invert
    G = _tiny_G("none")
    x = torch.rand(2, 1, 32, 64)
    # num_code == 1: the three multi-code arguments stay at their defaults
    for kw in (dict(composition_layer=2), dict(alpha=torch.ones(2, 1, 8)), dict(alpha_lr=1e-2),
               dict(num_code=1, composition_layer="2")):
        with pytest.raises(ValueError):
            invert(G, x, x, **kw)
    with pytest.raises(ValueError):
        invert(G, x, x, num_code=4)                      # composition_layer is required
    for n in (0, 65, 2.5):
        with pytest.raises(ValueError):
            invert(G, x, x, num_code=n, composition_layer=2)
    with pytest.raises(NotImplementedError):
        invert(G, x, x, num_code=4, composition_layer="1.1")
    # the cap on the lower batch: scans x codes <= 4096
    assert check_multi_code(64, 3, None, 1e-3, B=64) == 3
    with pytest.raises(ValueError, match="4096"):
        check_multi_code(64, 3, None, 1e-3, B=65)
    big = torch.rand(2049, 1, 32, 64)
    with pytest.raises(ValueError, match="4096"):
        invert(G, big, big, num_code=2, composition_layer=0)
    assert check_multi_code(1, None, None, 1e-3) is None


def test_cli_arguments_and_csv_columns():
    from dusty_gan_amd import evaluate_reconstruction as E
    base = ["--model-path", "m.pth", "--config-path", "c.yaml"]
    assert E.COLUMNS == REF_COLUMNS
    a = E.parse_args(base)
    assert (a.num_code, a.composition_layer) == (1, None)
    a = E.parse_args(base + ["--num-code", "4", "--composition-layer", "backbone.2", "--batch-size", "8"])
    assert (a.num_code, a.composition_layer, a.batch_size) == (4, "backbone.2", 8)
    for bad in (["--num-code", "4"], ["--composition-layer", "2"], ["--num-code", "65", "--composition-layer", "2"],
                ["--num-code", "4", "--composition-layer", "backbone.2.1"]):
        with pytest.raises(SystemExit):
            E.parse_args(base + bad)
    assert E.scans_per_pass(512, 1) == 512 and E.scans_per_pass(512, 4) == 512
    assert E.scans_per_pass(512, 16) == 256 and E.scans_per_pass(512, 64) == 64 and E.scans_per_pass(2, 64) == 2
    assert "--num-code" in E.__doc__ and "--composition-layer" in E.__doc__
