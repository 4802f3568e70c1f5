"""The matmul-precision switch on a host without a GPU: the Python API, the
C-ABI eligibility rule (include/hlhgat.h: hlhgat_gemm_bf16_eligible) and the
round-to-nearest-even helper of the CPU emulation.  Nothing here launches."""
import pytest
import torch

from bf16_ref import emulate_bf16_linear, emulated_linear, round_bf16


@pytest.fixture(autouse=True)
def _restore():
    import hlhgat
    yield
    hlhgat.set_matmul_precision("fp32")


def test_default_is_fp32():
    import hlhgat
    from hlhgat import _lib
    assert hlhgat.get_matmul_precision() == "fp32"
    assert _lib.LIB.hlhgat_get_gemm_precision() == 0


def test_set_get_and_context_restore():
    import hlhgat
    from hlhgat import _lib
    hlhgat.set_matmul_precision("bf16")
    assert hlhgat.get_matmul_precision() == "bf16"
    assert _lib.LIB.hlhgat_get_gemm_precision() == 1
    with hlhgat.matmul_precision("fp32"):
        assert hlhgat.get_matmul_precision() == "fp32"
        with hlhgat.matmul_precision("bf16"):
            assert hlhgat.get_matmul_precision() == "bf16"
        assert hlhgat.get_matmul_precision() == "fp32"
    assert hlhgat.get_matmul_precision() == "bf16"
    hlhgat.set_matmul_precision("fp32")
    with pytest.raises(KeyError):
        with hlhgat.matmul_precision("bf16"):
            assert hlhgat.get_matmul_precision() == "bf16"
            raise KeyError("leaves the context")
    assert hlhgat.get_matmul_precision() == "fp32"


def test_unknown_names_raise():
    import hlhgat
    with pytest.raises(ValueError):
        hlhgat.set_matmul_precision("fp16")
    with pytest.raises(ValueError):
        with hlhgat.matmul_precision("fp16"):
            pass
    assert hlhgat.get_matmul_precision() == "fp32"
    from hlhgat import _lib
    assert _lib.LIB.hlhgat_set_gemm_precision(2) == 1  # HLHGAT_EINVAL
    assert b"set_gemm_precision" in _lib.LIB.hlhgat_last_error()
    assert _lib.LIB.hlhgat_get_gemm_precision() == 0


class _Probe(torch.nn.Module):
    """A CPU model that records the precision its forward runs under."""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(8, 4)
        self.seen = []

    def forward(self, x):
        import hlhgat
        self.seen.append(hlhgat.get_matmul_precision())
        return self.lin(x)


def test_steps_accept_the_argument_on_a_cpu_model():
    import hlhgat
    from hlhgat.train import InferStep, TrainStep
    x, y = torch.randn(5, 8), torch.randn(5, 4)
    m = _Probe()
    step = TrainStep(m, lambda o, b: torch.nn.functional.mse_loss(o, y), graphs=False,
                     matmul_precision="bf16")
    assert step.matmul_precision == "bf16"
    assert torch.isfinite(step(x))
    assert m.seen == ["bf16"] and hlhgat.get_matmul_precision() == "fp32"
    inf = InferStep(m, graphs=False, matmul_precision="bf16")
    inf(x)
    assert m.seen == ["bf16", "bf16"] and hlhgat.get_matmul_precision() == "fp32"
    # None: the global value at construction, fixed for the object's life
    with hlhgat.matmul_precision("bf16"):
        late = InferStep(m, graphs=False)
    assert late.matmul_precision == "bf16"
    late(x)
    assert m.seen[-1] == "bf16"
    assert InferStep(m, graphs=False).matmul_precision == "fp32"
    with pytest.raises(ValueError):
        InferStep(m, graphs=False, matmul_precision="fp16")
    with pytest.raises(ValueError):
        TrainStep(m, lambda o, b: o.sum(), graphs=False, matmul_precision="tf32")


def test_eligibility_rule():
    import hlhgat
    ok = hlhgat.gemm_bf16_eligible
    assert ok([8], N=64)
    assert ok([64, 64, 64], N=64)
    assert not ok([36, 100], N=64)
    assert not ok([18], N=64)
    assert not ok([64], N=64, aligned16=False)
    assert ok([64], ld=[72], N=64)
    assert not ok([64], ld=[66], N=64)
    assert not ok([64], ld=[60], N=64)   # a stride below the width
    assert not ok([64], N=1) and not ok([64], N=0)
    assert ok([8] * 16, N=4) and not ok([8] * 17, N=4)  # HLHGAT_MAX_BLOCKS
    assert hlhgat.gemm_precision_stats(reset=True) == (0, 0)


def test_round_bf16_ties_to_even():
    t = torch.tensor([257., 259., -259., 256., 258., 1.0, 300.])
    assert round_bf16(t).tolist() == [256., 260., -260., 256., 258., 1.0, 300.]


def test_emulated_linear_rounds_as_the_contract_says():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(7, 16, generator=g, requires_grad=True)
    w = torch.randn(12, 16, generator=g, requires_grad=True)
    b = torch.randn(12, generator=g, requires_grad=True)
    go = torch.randn(7, 12, generator=g)
    with emulate_bf16_linear():
        y = torch.nn.functional.linear(x, w, b)
    y.backward(go)
    xr, wr, gr = (round_bf16(t.detach()).double() for t in (x, w, go))
    assert torch.equal(y.detach(), (xr @ wr.t() + b.detach().double()).float())
    assert torch.equal(x.grad, (gr @ wr).float())
    assert torch.equal(w.grad, (gr.t() @ xr).float())
    assert torch.equal(b.grad, go.double().sum(0).float())
    # an ineligible width keeps torch's fp32 Linear
    x18, w18 = torch.randn(3, 18, generator=g), torch.randn(4, 18, generator=g)
    plain = torch.nn.functional.linear(x18, w18)
    with emulate_bf16_linear():
        assert torch.equal(torch.nn.functional.linear(x18, w18), plain)
    assert torch.equal(emulated_linear(x18, w18), (round_bf16(x18).double()
                                                   @ round_bf16(w18).double().t()).float())
