"""The operand table of the GEMM epilogues (pixelrec_amd/csrc/gemm_epi.cuh: PXR_EPI_TABLE, epi_operands_ok) against the Python
restatement (tests/gemm_epi_restate.py: HAS_BIAS, READS_AUX, WRITES_AUX): every GEMM entry point must refuse an epilogue whose
bias or aux operand is missing, with PXR_ERR_BAD_ARG and a message that names the entry and the operand -- before anything is
launched, so this runs without a GPU (fake, 16-byte aligned, non-null addresses; only rejected calls are made).  The other
direction -- an operand the epilogue does not need may be None -- is held by tests/test_gpu_gemm_epilogues.py, which passes None
for each of them."""
import pytest

from tests import gemm_epi_restate as R

BAD_ARG = -1
ONE = 16                                                    # a non-null, 16-byte aligned address
M = N = K = 32
# the epilogues each operand flavour is instantiated for (b_kc = 1: forward, b_kc = 0: input gradient)
FWD = [R.EPI_NONE, R.EPI_BIAS, R.EPI_BIAS_GELU, R.EPI_BIAS_GELU_GRAD, R.EPI_BIAS_ADD, R.EPI_BIAS_QGELU_GRAD, R.EPI_BIAS_RELU,
       R.EPI_BIAS_ACT_GRAD]
BWD = [R.EPI_NONE, R.EPI_ADD, R.EPI_MUL]
FLAVOURS = {"pxr_gemm_f32": {1: FWD, 0: BWD + [R.EPI_MUL_DGELU]},
            "pxr_gemm_planes_f32": {1: FWD + [R.EPI_BIAS_QGELU], 0: BWD},
            "pxr_gemm_h2_f32": {1: FWD + [R.EPI_BIAS_QGELU], 0: BWD}}


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as entry
    from pixelrec_amd import lib

    entry.build()
    return lib.load()


def _call(L, entry, b_kc, epi, bias, aux):
    if entry == "pxr_gemm_f32":
        return L.pxr_gemm_f32(1, b_kc, M, N, K, ONE, K, ONE, K if b_kc else N, ONE, N, epi, bias, aux, N, None, 0, 0, 0, None)
    rows, stride = 32, 32 * 32                              # one panel of 32 rows x 32 columns per plane
    if entry == "pxr_gemm_planes_f32":
        return L.pxr_gemm_planes_f32(b_kc, M, N, K, ONE, stride, rows, ONE, stride, rows, ONE, N, epi, bias, aux, N, None, 0, 0, 0, 0, None)
    return L.pxr_gemm_h2_f32(b_kc, M, N, K, ONE, stride, rows, 0, None, ONE, stride, rows, 0, None, ONE, N, epi, bias, aux, N, None, 0, 0,
                             0, None, 0, 0, None)


@pytest.mark.parametrize("entry", sorted(FLAVOURS))
def test_every_entry_refuses_an_epilogue_whose_operand_is_missing(L, entry):
    calls = 0
    for b_kc, epis in FLAVOURS[entry].items():
        for epi in epis:
            what = f"{entry} b_kc={b_kc} epilogue {epi}"
            if epi in R.HAS_BIAS:
                assert _call(L, entry, b_kc, epi, None, ONE) == BAD_ARG, what + ": a null bias was accepted"
                err = L.pxr_last_error()
                assert entry.encode() in err and b"bias" in err, (what, err)
                calls += 1
            if epi in R.READS_AUX or epi in R.WRITES_AUX:
                assert _call(L, entry, b_kc, epi, ONE, None) == BAD_ARG, what + ": a null aux was accepted"
                err = L.pxr_last_error()
                assert entry.encode() in err and b"aux" in err, (what, err)
                calls += 1
    # (KC,KC): 7 or 8 bias + 5 aux epilogues; (KC,XC): 2 or 3 aux epilogues
    assert calls == {"pxr_gemm_f32": 7 + 5 + 3, "pxr_gemm_planes_f32": 8 + 5 + 2, "pxr_gemm_h2_f32": 8 + 5 + 2}[entry]
