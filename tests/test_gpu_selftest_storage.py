"""What the storage checks of the GPU self-test cover (native/egpu_selftest.hip:
the LDS march of selftest_kernel and hbm_pattern_kernel), on a real MI355X.

test_gpu_selftest.py shows that each check passes on a healthy GPU and sees
one corruption at one place. Here the place moves: the bytes the memory check
writes are compared with the numpy oracle of test_selftest_ref.py, and a
single flipped bit is put at every position a cheaper verify loop would skip
(word 3 of an element, the ends of a grid stride, the tail element, the last
word, the word the verifying thread index wraps at, the single word of a
second LDS stride), in the pattern pass and in the complement pass. Each must
be reported, exactly once, at exactly that place.

Every case is one or two launches of one to 64 workgroups. No test provokes a
fault, a hang or a timeout: every corruption is a data flip at a position the
library validated against the sizes of the same call.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _gpu_present():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


if not _gpu_present():
    pytest.skip("no AMD GPU present", allow_module_level=True)

from elastic_gpu_agent_amd.isolation import probes  # noqa: E402

from test_selftest_ref import hbm_words  # noqa: E402

SEED = 0x5EED1234
# 65,537 elements: the production grid is 64 workgroups of 256 threads, one
# grid stride is 64 * 256 * 16 = 262,144 bytes, and the fifth stride holds
# the one tail element
BUF = (1 << 20) + 16
STRIDE = 262144
ONE = 16  # one element: 255 of the 256 threads have nothing to do
RAGGED = 16 * 1023  # one workgroup, three full strides and a fourth of 255
SIZES = [ONE, RAGGED, BUF]


@pytest.fixture(scope="module")
def expected4():
    return probes.selftest_expected(SEED, 4)


@pytest.fixture(scope="module")
def pattern():
    """The oracle's words of the largest buffer; a smaller one is a prefix."""
    with np.errstate(over="ignore"):
        words = hbm_words(0, BUF // 16, SEED)
    words.setflags(write=False)
    return words


# ---------------------------------------------------------------- memory image

@pytest.mark.parametrize("march_pass", [0, 1])
@pytest.mark.parametrize("hbm_bytes", SIZES)
def test_memory_image_equals_oracle(pattern, hbm_bytes, march_pass):
    """A wrong word order inside the uint4, a skipped tail or a truncated
    index shows here as a wrong byte."""
    image = probes.selftest_hbm_image(0, hbm_bytes, SEED, march_pass)
    assert len(image) == hbm_bytes
    want = pattern[: hbm_bytes // 4] ^ np.uint32(0xFFFFFFFF if march_pass else 0)
    got = np.frombuffer(image, dtype="<u4")
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, f"{wrong.size} wrong words, first at byte {4 * wrong[0]}"
    assert image == want.astype("<u4").tobytes()


# ------------------------------------------------------------ memory placement

PLACES = [(BUF, off) for off in (0, 12, STRIDE - 4, STRIDE, 1 << 20, (1 << 20) + 12)]
PLACES += [(ONE, 0), (ONE, 12), (RAGGED, RAGGED - 4)]


@pytest.mark.parametrize("corrupt_pass", [0, 1])
@pytest.mark.parametrize("hbm_bytes, offset", PLACES)
def test_one_corrupt_word_is_found_where_it_is(hbm_bytes, offset, corrupt_pass):
    rep = probes.selftest_hbm(0, hbm_bytes, SEED, corrupt=[offset], corrupt_pass=corrupt_pass)
    print(rep)
    assert rep["hbm_miscompares"] == 1
    assert rep["hbm_first_bad_offset"] == offset
    assert rep["hbm_status"] == "failed"
    assert rep["hbm_bytes_checked"] == hbm_bytes


# ----------------------------------------------------------- memory accounting

@pytest.mark.parametrize("corrupt_pass", [0, 1])
@pytest.mark.parametrize("element", [4096, STRIDE + 16, 1 << 20])
def test_four_words_of_one_element(element, corrupt_pass):
    rep = probes.selftest_hbm(0, BUF, SEED, corrupt=[element + 4 * k for k in (2, 0, 3, 1)],
                              corrupt_pass=corrupt_pass)
    print(rep)
    assert rep["hbm_miscompares"] == 4
    assert rep["hbm_first_bad_offset"] == element
    assert rep["hbm_status"] == "failed"


@pytest.mark.parametrize("corrupt_pass", [0, 1])
def test_scattered_words_count_and_lowest_offset(corrupt_pass):
    """Four threads of four workgroups report: the count adds up and the
    lowest offset wins, whichever order they ran in."""
    rep = probes.selftest_hbm(0, BUF, SEED, corrupt=[(1 << 20) + 12, 4096, 8, STRIDE],
                              corrupt_pass=corrupt_pass)
    print(rep)
    assert rep["hbm_miscompares"] == 4
    assert rep["hbm_first_bad_offset"] == 8
    assert rep["hbm_status"] == "failed"


@pytest.mark.parametrize("hbm_bytes", SIZES)
def test_memory_check_alone_passes_clean(hbm_bytes):
    rep = probes.selftest_hbm(0, hbm_bytes, SEED)
    print(rep)
    assert rep["hbm_miscompares"] == 0 and rep["hbm_first_bad_offset"] == 0
    assert rep["hbm_status"] == "ok" and rep["hbm_bytes_checked"] == hbm_bytes


# --------------------------------------------------------------- LDS placement

# (lds_bytes, word). Word w is written by thread w % 256 and verified by
# thread (w - 67) % 256, which wraps between words 66 and 67.
LDS_PLACES = [(1024, w) for w in (0, 63, 64, 255)]  # one word per thread
LDS_PLACES += [(1028, 256)]  # the only word of the second stride
LDS_PLACES += [(32768, w) for w in (0, 66, 67, 255, 8191)]
LDS_PLACES += [(163840, w) for w in (0, 40959)]  # the CU's whole LDS


@pytest.mark.parametrize("march_pass", [0, 1])
@pytest.mark.parametrize("lds_bytes, word", LDS_PLACES)
def test_one_flipped_lds_word_is_found(expected4, lds_bytes, word, march_pass):
    inject = ("lds", 1, word, march_pass)
    recs = probes.selftest_records(0, blocks=3, rounds=4, lds_bytes=lds_bytes, seed=SEED,
                                   _inject=inject)
    assert len(recs) == 12
    for wave, (cu, int_sig, fma_sig, mfma_sig, lds_bad) in enumerate(recs):
        assert cu != 0xFFFFFFFF, f"wave {wave} wrote no record"
        assert (int_sig, fma_sig, mfma_sig) == expected4[wave], f"signatures, wave {wave}"
        assert lds_bad == (1 if wave // 4 == 1 else 0), f"lds_bad, wave {wave}"
    rep = probes.selftest(0, blocks=3, rounds=4, lds_bytes=lds_bytes, hbm_bytes=ONE, seed=SEED,
                          _inject=inject)
    print(rep)
    assert rep["bad_waves"] == 4 and rep["waves_run"] == 12
    assert rep["bad_kinds"] == probes.SELFTEST_KINDS["lds"]
    assert rep["n_bad_cus"] == 1 and len(rep["bad_cus"]) == 1
    assert rep["hbm_miscompares"] == 0 and rep["hbm_status"] == "ok"


# ------------------------------------------------------------ clean edge sizes

@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("lds_bytes", [1024, 1028])
def test_clean_pass_smallest_sizes(lds_bytes, blocks):
    rep = probes.selftest(0, blocks=blocks, rounds=4, lds_bytes=lds_bytes, hbm_bytes=ONE,
                          seed=SEED)
    print(rep)
    assert rep["bad_waves"] == 0 and rep["bad_kinds"] == 0 and rep["n_bad_cus"] == 0
    assert rep["waves_run"] == 4 * blocks and rep["lds_bytes"] == lds_bytes
    assert rep["hbm_miscompares"] == 0 and rep["hbm_status"] == "ok"
    assert rep["hbm_bytes_checked"] == ONE
