"""conv_s1r's cold vector-memory instructions (engine option `coldyw`): the look-ahead LDS-DMA pieces issued by the
SIMD's younger waves alone (1), and on top of that the first band of a workgroup run while its weights arrive (2, the default),
against the schedule before both (0).  The same bytes reach the same LDS addresses and registers and the arithmetic is untouched,
so every comparison here is torch.equal between the schedules on one engine."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}


def _engine(state_dict, B, dtype, **opts):
    from flope_amd.engine import PoseEngine
    e = PoseEngine(224, 224, B, dtype)
    for k, v in opts.items():
        e.set_option(k, v)
    e.load_state_dict(state_dict)
    return e


def _stages(e, x, coldyw):
    B = x.shape[0]
    e.set_option("coldyw", coldyw)
    r9, _ = e.forward(x)
    torch.cuda.synchronize()
    kernels = [k for _, k, _ in e.launch_info(B)]
    assert sum("conv_s1r_kernel" in k for k in kernels) == 3, kernels
    return {"layer2.0": e.read_stage("layer2.0", B).cpu(), "layer2.1": e.read_stage("layer2.1", B).cpu(), "r9": r9.cpu()}


# B = 3: 21 bands, one per workgroup -- the look-ahead of every workgroup points past the end.  B = 80: 560 bands on one workgroup
# per CU -- two or three bands each (buffer alternation, unequal walks); as two slices of 40, one or two.  dsfuse = 0: the block's
# shortcut is its own launch and layer2.0.conv2 is the residual form of the kernel.
@pytest.mark.parametrize("B,streams,opts", [(3, 1, {}), (3, 1, {"dsfuse": 0}), (80, 1, {}), (80, 2, {})],
                         ids=["B3", "B3-dsfuse0", "B80-1slice", "B80-2slices"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_cold_load_schedules_move_no_bit(state_dict, dtype, B, streams, opts):
    x = torch.rand(B, 224, 224, 3, generator=torch.Generator().manual_seed(300 + B)).to(TDT[dtype]).cuda()
    e = _engine(state_dict, B, dtype, streams=streams, **opts)
    old = _stages(e, x, 0)
    news = [_stages(e, x, v) for v in (1, 2)]
    e.close()
    assert float(old["layer2.1"].abs().max()) > 0
    for new in news:
        for name in old:
            assert torch.equal(old[name], new[name]), (name, float((old[name].float() - new[name].float()).abs().max()))

