"""The launch shapes the library picks by size, restated as pure functions (csrc/pnp_solver_abi.inc epnp_ransac_launch,
launch_epnp_stages, pick_wpo, widen_for_large_tiles, lm_launch_waves), and the case list of tests/test_gpu_launch_regimes.py.
The choices change the work, never a result: the GPU tests run every case against the oracle, and check this restatement of the
wave count against the library's own (mr_debug_launch_waves)."""

EP_MAX_ITERS = 30          # kEpMaxIters
EP_ROUND2_QUADS = 32       # kEpRound2Quads
SIMDS_PER_CU = 4
RED_N, MSG, HYP = 32, 20, 32      # kRedN, kMsg, kHyp (lds_bytes)
MI355X = dict(cus=256, lds_per_cu=160 * 1024)
ELEM = {'fp16': 2, 'fp32': 4, 'fp64': 8}


def pick_wpo(objects, P, cus):
    slots = cus * SIMDS_PER_CU * 4
    w = 1
    while w < 4 and objects * w * 2 <= 2 * slots and P >= 64 * w * 2:
        w *= 2
    wp = 1
    while wp < 4 and P > 64 * wp * 8:
        wp *= 2
    return max(w, wp)


def lds_bytes_4waves(P, dtype):
    """lds_bytes(a, 4) as widen_for_large_tiles evaluates it (before the launcher sets nca / nla: both 0)."""
    n = 8 * (2 * 4 * RED_N + MSG) + 4 * HYP * 8 + 4 * 4 * HYP + 4 * 4 + 8 * P * ELEM[dtype] + 2 * 2 * ((P + 7) & ~7) + P
    return (n + 15) & ~15


def lm_waves(objects, P, dtype, after_init=True, dev=MI355X):
    """Waves per object of the LM / covariance launch over `objects` objects (lm_launch_waves)."""
    w = pick_wpo(objects, P, dev['cus'])
    if w == 4 and dtype != 'fp64' and P >= 64 * 8 * 2 and lds_bytes_4waves(P, 'fp16' if dtype == 'fp16' else 'fp32') * 3 > dev['lds_per_cu']:
        w = 8
    if after_init:                                 # the external-initialiser launch has 2, 4 and 8 waves only
        w = 2 if w < 2 else (4 if w == 3 else w)
    return w


def epnp_regime(objects, first_round=None):
    """The initialiser's launch shapes for a launch set of `objects` objects (all calls): first round, second round ('one' launch or
    'two' compact ones), lv_h of the hypothesis launches issued (first round, and second round when it takes two launches), lv_b."""
    first = first_round if first_round else (3 if objects >= 2048 else 10)
    first = max(1, min(EP_MAX_ITERS, first))
    lv = lambda quads: 4 if quads <= 1024 else (2 if quads <= 4096 else 0)
    if first >= EP_MAX_ITERS:
        round2 = 'none'
    elif EP_MAX_ITERS - first <= EP_ROUND2_QUADS and objects < 2048:
        round2 = 'one'
    else:
        round2 = 'two'
    lv_h = (lv(objects * first),) + ((lv(objects * (EP_MAX_ITERS - first)),) if round2 == 'two' else ())
    lv_b = 4 if objects <= 512 else (2 if objects < 2048 else 0)
    return dict(first=first, round2=round2, lv_h=lv_h, lv_b=lv_b)


def regime(objects, calls, P, dtype, lm='fused', dev=MI355X, flow='epnp'):
    """Everything the host picks for `calls` equal calls of `objects` objects x P points (one call: calls = 1), LM launches as `lm` issues
    them ('fused' / 'grouped': one over the set; 'serial': one per call)."""
    total = objects * calls
    lm_objects = objects if lm == 'serial' else total
    if flow == 'k0':
        return dict(wpo=lm_waves(objects, P, dtype, after_init=False, dev=dev))
    return dict(epnp_regime(total), wpo=lm_waves(lm_objects, P, dtype, dev=dev))


# ---- the case list --------------------------------------------------------------------------------------------------------------
# (flow, B, P, dtype, layout): one call of B objects; 'epnp' = the default flow, 'k0' = the fast mode (the only flow with one wave)
B_EDGES = (1, 102, 103, 409, 410, 512, 513, 2047, 2048, 2049, 4096, 4097)
P_EDGES = (4, 5, 127, 128, 255, 256, 300, 512, 513, 1024, 1025)


def cases():
    out = [('epnp', B, 784, 'fp32', 'planar') for B in B_EDGES]
    for P in P_EDGES:                                  # the B values at which the wave count changes, on either side
        for B in (64, 2048, 2049, 4097):
            out.append(('epnp', B, P, 'fp32', 'contiguous' if P % 2 else 'planar'))
    out += [('epnp', 300, 784, 'fp16', 'planar'), ('epnp', 300, 784, 'fp64', 'contiguous'), ('epnp', 2049, 300, 'fp16', 'contiguous'),
            ('epnp', 64, 3136, 'fp16', 'planar'), ('epnp', 64, 3136, 'fp32', 'contiguous')]
    out += [('k0', 64, 127, 'fp32', 'planar'), ('k0', 4097, 300, 'fp32', 'contiguous'), ('k0', 2049, 300, 'fp32', 'planar'), ('k0', 64, 300, 'fp32', 'planar')]
    return out


B_BOUNDARIES = (102, 409, 512, 2047, 2048, 4096)          # a choice changes between B and B + 1
P_BOUNDARIES = (4, 127, 255, 512, 1024)
