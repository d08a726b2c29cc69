"""cov_symeig_rule_kernel (one thread per object, blocks of 64) at object counts around its block size: the synthetic-covariance check
of tests/test_gpu_parity.py::test_reference_eigenvalue_rule_for_ill_conditioned_hessians, part (a), through the C ABI with valid, cov
and eig_min_max in guarded, prefilled buffers, with and without eig_min_max, and with objects that enter invalid."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
COUNTS = (1, 63, 64, 65, 130)                    # a lone object, one short of a block, a block, one over, two blocks and two objects


def covariances(B, seed=12):
    """B float32 covariances cycling through part (a)'s kinds: condition numbers 1 ... 1e12, indefinite, NaN, identity"""
    rng = np.random.default_rng(seed)
    kinds = [1.0, 'nan', 1e2, 'indefinite', 1e5, 9e5, 'eye', 1.1e6, 1e7, 1e12]
    covs = []
    for i in range(B):
        kind = kinds[i % len(kinds)]
        q, _ = np.linalg.qr(rng.normal(size=(4, 4)))
        if kind == 'indefinite':
            covs.append(q @ np.diag([-1e-3, 1.0, 2.0, 3.0]) @ q.T)
        elif kind == 'nan':
            covs.append(np.full((4, 4), np.nan))
        elif kind == 'eye':
            covs.append(np.eye(4))
        else:
            cond = float(kind)
            lam = np.array([1.0, cond ** (1 / 3), cond ** (2 / 3), cond]) * rng.uniform(1e-4, 1e2)
            covs.append(q @ np.diag(lam) @ q.T)
    return np.stack(covs).astype(np.float32), [kinds[i % len(kinds)] for i in range(B)]


def run_abi(valid, cov, with_eigs, fill=0xFF):
    """mr_cov_symeig_rule with a guard element / row on each side of valid, cov and eig_min_max -> the three buffers as bits, code"""
    from monorun_amd import _lib
    B = len(valid)
    v = torch.full((B + 2,), fill, dtype=torch.uint8, device=DEV)
    v[1:-1] = torch.from_numpy(valid).to(DEV)
    c = torch.full(((B + 2) * 64,), fill, dtype=torch.uint8, device=DEV).view(torch.float32).view(B + 2, 16)
    c[1:-1] = torch.from_numpy(cov.reshape(B, 16)).to(DEV)
    e = torch.full(((B + 2) * 8,), fill, dtype=torch.uint8, device=DEV).view(torch.float32).view(B + 2, 2) if with_eigs else None
    code = _lib.load().mr_cov_symeig_rule(*_lib.pack('mr_cov_symeig_rule', valid=v[1:].data_ptr(), cov=c[1:].data_ptr(), B=B,
                                                     eig_min_max=None if e is None else e[1:].data_ptr()), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return v.cpu().numpy(), c.view(torch.int32).cpu().numpy(), None if e is None else e.view(torch.int32).cpu().numpy(), code


@pytest.mark.parametrize('enter_invalid', [False, True])
@pytest.mark.parametrize('B', COUNTS)
def test_rule_at_block_boundaries(orc, B, enter_invalid):
    from monorun_amd import _lib
    cov, kinds = covariances(B)
    valid = np.ones(B, np.uint8)
    enters = [i for i, k in enumerate(kinds) if k in (1.0, 'eye')] if enter_invalid else []      # objects with a good covariance that enter invalid
    valid[enters] = 0
    assert bool(enters) == enter_invalid
    r_valid, r_cov, r_lam = orc.cov_symeig_rule(valid, cov)
    assert not r_valid[enters].any() and np.array_equal(r_cov[enters], cov[enters])
    v, c, e, code = run_abi(valid, cov, True)
    word = np.int32(-1)
    assert code == 0 and v[0] == 0xFF and v[-1] == 0xFF and np.all(c[[0, -1]] == word) and np.all(e[[0, -1]] == word)
    got_valid, got_cov, got_lam = v[1:-1].astype(bool), c[1:-1].view(np.float32).reshape(B, 4, 4), e[1:-1].view(np.float32)
    # the eigenvalue test itself is compared away from its own threshold (float32 covariances: the ratio is known to ~1e-6 relative)
    ratio = r_lam[:, 0] / np.where(r_lam[:, 1] != 0, r_lam[:, 1], 1.0)
    clear = ~np.isfinite(ratio) | (np.abs(ratio / 1e-6 - 1.0) > 0.05)
    assert clear.sum() >= 0.8 * B and np.array_equal(got_valid[clear], r_valid[clear])
    same = got_valid == r_valid
    assert np.array_equal(got_cov[same], r_cov[same], equal_nan=True)
    assert not got_valid[enters].any() and np.array_equal(got_cov[enters], cov[enters])    # enters invalid with a good covariance: stays 0, untouched
    fin = np.isfinite(r_lam).all(1)
    assert np.allclose(got_lam[fin], r_lam[fin], rtol=1e-4, atol=1e-7 * np.abs(r_lam[fin]).max(1, keepdims=True))
    assert np.all(e[1:-1][fin] != word)                                                     # every object's pair is written
    for i, k in enumerate(kinds):
        if k in ('indefinite', 'nan', 1e7, 1e12):
            assert not got_valid[i] and np.array_equal(got_cov[i], np.eye(4, dtype=np.float32)), (i, k)
        elif k in (1.0, 1e2, 1e5, 9e5, 'eye') and i not in enters:
            assert got_valid[i] and np.array_equal(got_cov[i], cov[i]), (i, k)
    print(f'B {B}: {int(got_valid.sum())} kept, {len(enters)} enter invalid, {int((~clear).sum())} at the threshold not judged')
    v2, c2, e2, code2 = run_abi(valid, cov, False)                                          # eig_min_max = NULL: the same valid and cov
    assert code2 == 0 and e2 is None and np.array_equal(v2, v) and np.array_equal(c2, c)
    v3, c3, e3, code3 = run_abi(valid, cov, True, fill=0x00)
    assert code3 == 0 and np.array_equal(v3[1:-1], v[1:-1]) and np.array_equal(c3[1:-1], c[1:-1]) and np.array_equal(e3[1:-1], e[1:-1])
    assert v3[0] == 0 and v3[-1] == 0 and not c3[[0, -1]].any() and not e3[[0, -1]].any()
    assert _lib.load().mr_pnp_last_hip_error() == 0
