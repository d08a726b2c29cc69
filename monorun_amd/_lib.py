"""ctypes loader / builder for libmonorun_pnp.so: the C ABI that the headers of ``HEADERS`` declare (include/*.h, one per subsystem).

The library is built in-tree by hipcc for gfx950 (``build()``; also driven by
``__graft_entry__.build()``) and loaded with ctypes — cffi, which the reference uses
(/root/reference/monorun/ops/least_squares/setup.py:12-24), is not assumed to exist.
There is NO CPU fallback: if the library is missing or no HIP device is present the ops raise.
"""
import ctypes
import glob
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
SRC = os.path.join(_HERE, 'csrc', 'monorun_pnp.hip')
INCLUDE = os.path.join(_ROOT, 'include')
SO = os.environ.get('MR_PNP_SO') or os.path.join(_HERE, 'libmonorun_pnp.so')     # MR_PNP_SO: A/B-test another build of the library

# The public surface of the one library: key -> (header under include/, the entry points it declares in declaration order).  The tuples are
# written by hand: they pin the surface, so that a change to a header shows up as a change here (tests/test_capi_and_host.py).  A new
# subsystem adds one row, and `_stale`, `load` and the prototypes follow.  `pnp` is the cffi surface of INTEGRATION.md section 3 (with the
# reference's three host-buffer symbols of ext.h); the other headers are outside it.
HEADERS = {
    'pnp': ('monorun_pnp.h', (
        'mr_pnp_version', 'mr_pnp_error_string', 'mr_pnp_last_hip_error', 'mr_pnp_device_count', 'mr_pick_waves', 'mr_spin',
        'mr_pnp_uncert_batched', 'mr_epnp_ransac_batched', 'mr_epnp_workspace_bytes', 'mr_epnp_ransac_grouped', 'mr_pnp_uncert_from_init_batched',
        'mr_pnp_uncert_from_init_grouped', 'mr_pnp_uncert_from_epnp_grouped', 'mr_cov_symeig_rule', 'mr_pnp6_refine_batched',
        'mr_pnp_exact_hessian_batched', 'mr_pnp_uncert_backward_batched', 'pnp_uncert',
        'mr_noc_decode_batched', 'mr_pnp_from_head_batched', 'mr_roi_align_avg', 'mr_nms_bev_batched',
        'mr_bbox3d_overlaps_aligned', 'mr_uncert_projection', 'mr_uncert_projection_backward', 'mr_robust_kl_workspace_bytes', 'mr_robust_kl_loss',
        'mr_robust_kl_loss_backward',
        'mr_kitti_overlaps', 'mr_kitti_match_workspace_bytes', 'mr_kitti_match',
        'pnp_noc_uncert', 'pnp_noc_cov_uncert', 'mr_pnp_noc_batched')),
    'heads': ('monorun_heads.h', ('mr_score_head_forward',)),
    'train': ('monorun_train.h', ('mr_noc_decode_train', 'mr_noc_decode_train_backward')),                             # section 14
    'targets': ('monorun_targets.h', ('mr_noc_dense_target', 'mr_smooth_l1_mod_workspace_bytes', 'mr_smooth_l1_mod_loss',
                                      'mr_smooth_l1_mod_loss_backward')),                                               # section 15
    'global': ('monorun_global.h', ('mr_global_head_mc_workspace_bytes', 'mr_global_head_mc_forward')),                # section 16
    'carafe': ('monorun_carafe.h', ('mr_carafe_pack_forward', 'mr_carafe_backward_workspace_bytes', 'mr_carafe_pack_backward')),   # section 17
}
# The headers added since the table above was pinned to its six rows (tests/test_capi_and_host.py): the same form, walked after it by
# `_stale`, `load` and the prototypes; `exported_symbols()` without a key stays the list of ``HEADERS``.
EXTRA_HEADERS = {
    'roi': ('monorun_roi.h', ('mr_roi_extract_forward', 'mr_roi_extract_backward')),                                   # section 18
}
# Every later header goes here: the two tables above are pinned to their rows by tests, this one is open-ended by design and a new
# subsystem adds ONE ROW to it (each row is pinned by its own subsystem's test).  `_stale`, `load`, the prototypes, `header_path` and
# `exported_symbols(key)` walk all three tables (``all_header_keys``); `header_keys()` and a bare `exported_symbols()` stay what they were.
LATER_HEADERS = {
    'proposals': ('monorun_proposals.h', ('mr_proposal_decode', 'mr_nms_workspace_bytes', 'mr_nms_grouped')),        # section 19
    'bbox': ('monorun_bbox.h', ('mr_bbox_head_rank', 'mr_bbox_head_select', 'mr_bbox_head_workspace_bytes', 'mr_bbox_head_detect')),   # section 20
    'assign': ('monorun_assign.h', ('mr_assign_workspace_bytes', 'mr_assign_max_iou')),                               # section 21
    'fpn': ('monorun_fpn.h', ('mr_fpn_topdown_forward', 'mr_fpn_topdown_backward')),                                   # section 22
    'backbone': ('monorun_backbone.h', ('mr_bn_act_forward', 'mr_bn_act_backward_workspace_bytes', 'mr_bn_act_backward',
                                        'mr_bn_relu_maxpool_forward')),                                                 # section 23
    'result3d': ('monorun_result3d.h', ('mr_result3d_nms',)),                                                          # section 24
    'roi_train': ('monorun_roi_train.h', ('mr_roi_train_positives',)),                                                 # section 25
    'image': ('monorun_image.h', ('mr_image_prepare',)),                                                               # section 26
}


def _table(key):
    for table in (HEADERS, EXTRA_HEADERS, LATER_HEADERS):
        if key in table:
            return table[key]
    raise KeyError(key)


def header_keys():
    """The keys of the two pinned tables: ``HEADERS``, then ``EXTRA_HEADERS``."""
    return tuple(HEADERS) + tuple(EXTRA_HEADERS)


def all_header_keys():
    """The keys of every header: ``HEADERS``, ``EXTRA_HEADERS``, then ``LATER_HEADERS``."""
    return header_keys() + tuple(LATER_HEADERS)


def header_path(key):
    """The file of one of the headers of the three tables."""
    return os.path.join(INCLUDE, _table(key)[0])


def exported_symbols(key=None):
    """The pinned entry points of one header (of any table), or of all those of ``HEADERS`` in table order."""
    return _table(key)[1] if key is not None else tuple(n for _, names in HEADERS.values() for n in names)


MR_F32, MR_F16, MR_F64, MR_BF16 = 0, 1, 2, 3
MR_MEAN_AUTO, MR_MEAN_SEQUENTIAL, MR_MEAN_PAIRWISE, MR_MEAN_MASK = 0, 1, 2, 3          # MR_MEAN_MASK: the two bits of the istd mean's order
MR_NO_ISTD_MASK, MR_COV_NONE, MR_COV_CERES, MR_ANY_ORDER = 0x4, 0x8, 0x10, 0x20
MR_EPNP_REFIT_F32 = 0x40
MR_EPNP_DEFER_REFIT = 0x80
MR_EPNP_CV_EARLY_RETURN = 0x1000
MR_WAVES_SHIFT = 8
MR_LM_MAXIT_SHIFT = 16
MR_EPNP_FIRST_ROUND_SHIFT = 24
MR_IOU3D_GEOMETRIC_HEIGHT = 0x1
MR_SCORE_SIGMOID = 0x1

HIPCC_FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared']

_lib = None


def _stale():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    csrc = os.path.join(_HERE, 'csrc')
    deps = glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.inc')) + [header_path(k) for k in all_header_keys()]
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    """Compile the HIP library for gfx950 (cross-compiles without a GPU)."""
    if not force and not _stale():
        return SO
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    extra = os.environ.get('MR_HIPCC_EXTRA', '').split()
    cmd = [hipcc] + HIPCC_FLAGS + extra + ['-I', INCLUDE, SRC, '-o', SO]
    if verbose:
        print(' '.join(cmd))
    subprocess.check_call(cmd)
    return SO


def header_prototypes(path=None):
    """[(name, 'return type', ['arg type name', ...])] for every function the header declares (default: the `pnp` header, the cffi surface)."""
    src = open(path or header_path('pnp')).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    src = re.sub(r'//[^\n]*', ' ', src)
    src = '\n'.join(l for l in src.split('\n') if not l.lstrip().startswith('#') and 'extern "C"' not in l and l.strip() != '}')
    out = []
    for m in re.finditer(r'([A-Za-z_][\w\s\*]*?)\b(\w+)\s*\(([^()]*)\)\s*;', src):
        ret, name, args = ' '.join(m.group(1).split()), m.group(2), m.group(3)
        args = [' '.join(a.split()).replace('* ', '*') for a in args.split(',')] if args.strip() not in ('', 'void') else []
        out.append((name, ret, args))
    return out


def _all_prototypes():
    return [p for k in all_header_keys() for p in header_prototypes(header_path(k))]


_CTYPES = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t, 'int64_t': ctypes.c_int64}
_prototypes = None


def _ctype(name, ctype):
    """The ctypes type of a C type of the header.  A type this table does not know is an error, not a guess."""
    if '*' in ctype:
        return ctypes.c_void_p
    if ctype not in _CTYPES:
        raise TypeError(f'{name}: its header uses the type {ctype!r}, which the loader has no ctypes mapping for')
    return _CTYPES[ctype]


def _prototype(fn):
    """(restype, [argtypes], (argument names without the trailing stream), (names of the per-call pointer tables `T *const *`),
    frozenset of the names) of an `mr_*` entry point, as its header of ``HEADERS`` declares it.  The headers are read once."""
    global _prototypes
    if _prototypes is None:
        protos = {}
        for name, ret, args in _all_prototypes():
            if not name.startswith('mr_'):
                continue                                # the reference's cffi symbols of ext.h: declared by hand in load()
            assert name not in protos, f'{name}: declared twice'
            decl = [re.fullmatch(r'(.*?)(\w+)', a).groups() for a in args]
            names = tuple(n for _, n in decl)
            assert len(set(names)) == len(names), f'{name}: argument names repeat'
            protos[name] = (ctypes.c_char_p if ret == 'const char *' else _ctype(name, ret),
                            [_ctype(name, t.replace('const', '').strip()) for t, _ in decl],
                            names[:-1] if names[-1:] == ('stream',) else names, tuple(n for t, n in decl if t.count('*') == 2), frozenset(names))
        _prototypes = protos
    return _prototypes[fn]


def arg_names(fn):
    """The argument names of an entry point in ABI order, without the trailing `stream`."""
    return _prototype(fn)[2]


def table_args(fn):
    """The arguments a grouped entry point takes as per-call pointer tables (`T *const *`: one pointer per member)."""
    return _prototype(fn)[3]


def pack(fn, common={}, /, **named):
    """The argument list of `lib.<fn>(*args, stream)` in ABI order from arguments given by the header's names.  `common`: a dict the
    names missing from `named` are taken from (it may hold more than `fn` declares: another prototype's arguments, say).  TypeError
    for a name in `named` that `fn` does not declare and for a declared one that neither gives."""
    names = arg_names(fn)
    if not named.keys() <= _prototype(fn)[4]:
        raise TypeError(f'{fn}: unknown argument {sorted(set(named) - set(names))}')
    try:
        return [named[n] if n in named else common[n] for n in names]
    except KeyError as e:
        raise TypeError(f'{fn}: missing argument {e}') from None


def ptr(t):
    """data_ptr() of an optional tensor (None: a NULL argument)."""
    return t.data_ptr() if t is not None else None


def load():
    """Return the ctypes handle; raises if the library has not been built.  restype / argtypes of every `mr_*` entry point come
    from its prototype in its header of ``HEADERS`` (``_prototype``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO):
        raise RuntimeError(
            f'{SO} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950). monorun_amd has no CPU fallback.')
    lib = ctypes.CDLL(SO)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    for name, _, _ in _all_prototypes():
        if name.startswith('mr_'):
            f = getattr(lib, name)
            f.restype, argtypes = _prototype(name)[:2]
            if argtypes:
                f.argtypes = argtypes
    # development aids for the tests (in no public header, not in HEADERS)
    lib.mr_debug_launch_waves.restype = i32
    lib.mr_debug_launch_waves.argtypes = [i32, i32, i32, i32, i32]
    lib.mr_debug_block_sum.restype = i32
    lib.mr_debug_block_sum.argtypes = [i32, vp, vp, vp]
    # the reference's cffi signatures (ext.h): callers pass typed pointers
    dp = ctypes.POINTER(ctypes.c_double)
    lib.pnp_uncert.restype = None
    lib.pnp_uncert.argtypes = [dp, dp, dp, dp, dp, ctypes.POINTER(i32), dp, dp, dp, i32, dp]
    for name in ('pnp_noc_uncert', 'pnp_noc_cov_uncert'):
        f = getattr(lib, name)
        f.restype = None
        f.argtypes = [dp, dp, dp, dp, dp, dp, dp, ctypes.POINTER(i32), dp, i32, dp, ctypes.c_double]
    _lib = lib
    return lib


def check(code):
    if code != 0:
        lib = load()
        raise RuntimeError(f'libmonorun_pnp: {lib.mr_pnp_error_string(code).decode()} '
                           f'(code {code}, hip error {lib.mr_pnp_last_hip_error()})')


def call(fn, common={}, /, *, stream, **named):
    """Launch the entry point `fn` on `stream` (the raw hipStream_t handle) with its arguments given by the header's names (``pack``), and
    raise unless it returns MR_OK."""
    check(getattr(load(), fn)(*pack(fn, common, **named), stream))
