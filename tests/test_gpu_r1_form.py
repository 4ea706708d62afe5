"""The three forms of R1 at the image in the D phase (trainers/dcgan_amp.py `R1Form`), each reached on purpose: the step of
tests/test_gpu_configs.py::test_config1_plumbing_32x256_batch8_fp32 - 32x256 takes the one-launch turn-around by itself -
and the same step with `r1_form` patched to name a lower form (both are valid there: H * W = 8192 is a multiple of 1024).
Every form is held to the bounds that test holds the first one to, which come from the fp32 oracle."""
import pytest

from tests.test_gpu_configs import FP32, _check
from tests.test_gpu_step import run_both

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["TURNAROUND", "FUSED_ADJOINT", "THREE_PASS"])
def test_each_r1_form_stays_inside_the_fp32_bounds(name, monkeypatch):
    from dusty_gan_amd.trainers import dcgan_amp
    form = dcgan_amp.R1Form[name]
    if form is not dcgan_amp.R1Form.TURNAROUND:
        monkeypatch.setattr(dcgan_amp, "r1_form", lambda **kw: form)
    tr, state, res = run_both("none", (32, 256), 512, 64, 512, 8, amp=False, sync=True)
    assert tr.r1_form is form, tr.r1_form
    _check(res[0], tr, state, **FP32)
