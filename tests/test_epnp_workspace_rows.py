"""The hand-over workspace's last array: the re-fit's point list as a bit row per object (csrc/epnp_stages.inc: epnp_work_bytes, ep_fitbits), which
the LM launch that carries the re-fit loads with 8-byte loads.  mr_epnp_workspace_bytes against a restatement of the layout: it grows by exactly
the rows over the arrays that were there before, and every row starts on an 8-byte boundary, for odd P and for B that is no multiple of 8.  No GPU."""
import pytest

K_META, K_ITERS, K_SAMP, K_CAND_STRIDE = 12, 30, 28, 40


def _up(n, a=256):
    return (n + a - 1) // a * a


def _arrays_before(B, P):
    """(name, bytes) of the arrays up to spt, in layout order; every array starts on a 256-byte boundary."""
    nq, ps = B * K_ITERS, (P + 7) // 8 * 8
    return [('meta', 4 * K_META * B), ('samp', 4 * K_SAMP * nq), ('hrt', 8 * 12 * nq), ('cand', 2 * ps * B), ('fit', 2 * ps * B), ('prep_r', 8 * 24 * B),
            ('mtm_r', 8 * 144 * B), ('cand_r', 8 * K_CAND_STRIDE * B), ('cam', 4 * 4 * B), ('abt_r', 8 * 24 * B), ('spt', 2 * 5 * K_ITERS * B)]


@pytest.fixture(scope='module')
def lib():
    from monorun_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('B', [1, 7, 37, 100, 1024, 5120])
@pytest.mark.parametrize('P', [4, 5, 63, 64, 65, 129, 783, 784, 3137])
def test_workspace_grows_by_exactly_the_bit_rows(lib, B, P):
    before = sum(_up(n) for _, n in _arrays_before(B, P))
    words = (P + 63) // 64
    rows = 8 * words * B
    assert int(lib.mr_epnp_workspace_bytes(B, P)) == before + _up(rows), (B, P)
    # the rows start where the arrays before them end (a multiple of 256 from a 256-byte aligned workspace), one after the other, `words` 8-byte words each
    assert before % 256 == 0 and all((before + 8 * words * b) % 8 == 0 for b in (0, 1, B - 1))
    assert 64 * words >= P > 64 * (words - 1)
