"""The launch arithmetic of the grid-stride kernels, restated, and the shapes at which their loops take a second trip -- not a test:
test_grid_wrap_host.py holds the table to this arithmetic and to the grid_for(...) lines of the sources, test_grid_wrap_gpu.py runs
every row against the float64 reference its kernel already has.

Every elementwise kernel is launched with grid_for(work, 256, cap) workgroups of 256 threads (csrc/host_common.h): cap 2048, or 4096
in transformer.hip and aoa_ctx.hip.  With T = cap * 256 threads a launch covers T items per trip of its
`for (i = tid; i < n; i += gridDim.x * blockDim.x)` loop, so a second trip runs only when n > T.  adam2_kernel, optim_kernel and
ema_kernel take two quads per trip (q0 and q1 = q0 + stride, advancing by 2 * stride): q0 enters trip 2 past 2 T quads, q1 is live
there past 3 T.
"""
import os
import re

PER_BLOCK = 256
CAP, CAP4 = 2048, 4096
T = CAP * PER_BLOCK                 # 524 288 threads at the default cap
T4 = CAP4 * PER_BLOCK               # 1 048 576 in transformer.hip / aoa_ctx.hip
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'imagecaptioning', 'pytorch_amd', 'csrc')
MINIMAL = 1024                      # a row exceeds its threshold by at most this many loop items


def grid_for(work, per_block=PER_BLOCK, cap=CAP):
    """csrc/host_common.h grid_for"""
    return max(1, min(cap, (work + per_block - 1) // per_block))


# ------------------------------------------------------------------------------------------------ per-launcher arithmetic
# name -> (source file, the kernel named on the grid_for line or None, the argument text of grid_for, cap,
#          shape -> work handed to grid_for, shape -> items the loop walks).  `shape` is a dict.
def _optim_split(s):
    """optim_launch / ema_launch: (head, quads, scalars) of a range of n elements whose buffers start at the given element offsets"""
    n, offs = s['n'], s['offs']
    head = n
    if len(set(o % 4 for o in offs)) == 1:
        head = min(n, (4 - offs[0] % 4) % 4)
    quads = (n - head) // 4
    return head, quads, n - 4 * quads


def _optim_work(s):
    _, quads, scalars = _optim_split(s)
    return max(quads // 2 + 1, scalars)


LAUNCHERS = {
    'adam2_kernel': ('pointwise.hip', 'adam2_kernel', 'quads / 2 + 1', CAP, lambda s: s['count'] // 4 // 2 + 1, lambda s: s['count'] // 4),
    'adam_kernel': ('pointwise.hip', 'adam_kernel', '(size_t)count / 4 + 4', CAP, lambda s: s['count'] // 4 + 4, lambda s: s['count'] // 4),
    # optim.hip: work = quads / 2 + 1 > scalars ? quads / 2 + 1 : scalars, one line above each launch.  NOT guarded: the source
    # check reads grid_for( lines only and sees the argument `work`; a change to that expression leaves _optim_work stale without
    # a failure here (the same holds for `quads` of region_norm.hip and `work` of beam.hip)
    'optim_kernel': ('optim.hip', 'optim_kernel', 'work', CAP, _optim_work, lambda s: _optim_split(s)[1]),
    'optim_kernel scalars': ('optim.hip', 'optim_kernel', 'work', CAP, _optim_work, lambda s: _optim_split(s)[2]),
    'ema_kernel': ('optim.hip', 'ema_kernel', 'work', CAP, _optim_work, lambda s: _optim_split(s)[1]),
    'relu_mask_bwd': ('pointwise.hip', 'relu_mask_bwd_kernel', '(size_t)count', CAP, lambda s: s['count'], lambda s: s['count']),
    'relu_scale_bwd': ('pointwise.hip', 'relu_scale_bwd_kernel', '(size_t)count / 4', CAP, lambda s: s['count'] // 4, lambda s: s['count'] // 4),
    'dropout_mask': ('pointwise.hip', 'dropout_mask_kernel', '(size_t)(count + 3) / 4', CAP, lambda s: (s['count'] + 3) // 4,
                     lambda s: (s['count'] + 3) // 4),
    'dropout_masks': ('pointwise.hip', 'dropout_masks_kernel', '(most + 3) / 4', CAP, lambda s: (max(s['counts']) + 3) // 4,
                      lambda s: (max(s['counts']) + 3) // 4),
    'bn_apply': ('region_norm.hip', 'bn_apply_kernel', 'quads', CAP, lambda s: s['rows'] * ((s['D'] + 3) // 4),
                 lambda s: s['rows'] * ((s['D'] + 3) // 4)),
    'bn_bwd_dx': ('region_norm.hip', 'bn_bwd_dx_kernel', 'quads', CAP, lambda s: s['rows'] * ((s['D'] + 3) // 4),
                  lambda s: s['rows'] * ((s['D'] + 3) // 4)),
    'glu_fwd': ('transformer.hip', 'glu_fwd_kernel', '(size_t)M * R, 256, 4096', CAP4, lambda s: s['M'] * s['R'], lambda s: s['M'] * s['R']),
    'glu_fwd_fused': ('transformer.hip', 'glu_fwd_fused_kernel', '(size_t)M * (R / 4), 256, 4096', CAP4, lambda s: s['M'] * (s['R'] // 4),
                      lambda s: s['M'] * (s['R'] // 4)),
    'glu_bwd': ('transformer.hip', 'glu_bwd_kernel', '(size_t)M * R, 256, 4096', CAP4, lambda s: s['M'] * s['R'], lambda s: s['M'] * s['R']),
    'split_halves': ('transformer.hip', 'split_halves_kernel', '(size_t)M * 2 * R, 256, 4096', CAP4, lambda s: s['M'] * 2 * s['R'],
                     lambda s: s['M'] * 2 * s['R']),
    'embed_pe_fwd': ('transformer.hip', 'embed_pe_fwd_kernel', '(size_t)N * T * D, 256, 4096', CAP4, lambda s: s['N'] * s['T'] * s['D'],
                     lambda s: s['N'] * s['T'] * s['D']),
    'embed_pe_bwd': ('transformer.hip', 'embed_pe_bwd_kernel', '(size_t)N * T * D, 256, 4096', CAP4, lambda s: s['N'] * s['T'] * s['D'],
                     lambda s: s['N'] * s['T'] * s['D']),
    'meanpool_bwd': ('transformer.hip', 'meanpool_bwd_kernel', '(size_t)B * K * D, 256, 4096', CAP4, lambda s: s['B'] * s['K'] * s['D'],
                     lambda s: s['B'] * s['K'] * s['D']),
    'relu_bwd_add': ('aoa_ctx.hip', 'relu_bwd_add_kernel', '(size_t)M * R, 256, 4096', CAP4, lambda s: s['M'] * s['R'], lambda s: s['M'] * s['R']),
    # capmi_ctx_fwd_fused: `const dim3 grid(grid_for(...))`, the three kinds launch with it
    'ctx_fwd_fused': ('aoa_ctx.hip', None, '(size_t)s->M * (s->R / 4), 256, 4096', CAP4, lambda s: s['M'] * (s['R'] // 4),
                      lambda s: s['M'] * (s['R'] // 4)),
    # capmi_rows_narrow: `const int grid = grid_for(...)`, both dtypes launch with it, THREADS (resident_threads()) per workgroup;
    # the loop walks the 16-byte stores of 8 elements behind a scalar head of up to 7 (dst_off: elements past a 16-byte boundary)
    'rows_narrow': ('resident.hip', None, '(size_t)(count / 8 + 1), THREADS', CAP, lambda s: s['count'] // 8 + 1,
                    lambda s: (s['count'] - min(s['count'], (8 - s['dst_off'] % 8) % 8)) // 8),
    # capmi_lineage_gather: work = L * rows_dst * (C_a / 4 + C_b / 4) float4 moves, or L * rows_dst * (C_a + C_b) scalar ones
    'lineage_gather float4': ('beam.hip', 'lineage_gather_kernel<float4>', 'work', CAP,
                              lambda s: s['L'] * s['rows_dst'] * (s['Ca'] // 4 + s['Cb'] // 4), lambda s: s['L'] * s['rows_dst'] * (s['Ca'] // 4 + s['Cb'] // 4)),
    'lineage_gather float': ('beam.hip', 'lineage_gather_kernel<float>', 'work', CAP,
                             lambda s: s['L'] * s['rows_dst'] * (s['Ca'] + s['Cb']), lambda s: s['L'] * s['rows_dst'] * (s['Ca'] + s['Cb'])),
}


def resident_threads():
    """THREADS of resident.hip, the workgroup size of rows_narrow_kernel's launch"""
    with open(os.path.join(CSRC, 'resident.hip')) as f:
        return int(re.search(r'constexpr int THREADS = (\d+);', f.read()).group(1))
TWO_QUADS = ('adam2_kernel', 'optim_kernel', 'ema_kernel')          # q0 / q1 = q0 + stride per trip, advancing by 2 * stride


def stride(name, shape):
    _, _, _, cap, work, _ = LAUNCHERS[name]
    return grid_for(work(shape), PER_BLOCK, cap) * PER_BLOCK


def items(name, shape):
    return LAUNCHERS[name][5](shape)


def trips(name, shape):
    """trips of the kernel's outer loop that at least one thread takes"""
    per_trip = stride(name, shape) * (2 if name in TWO_QUADS else 1)
    return (items(name, shape) + per_trip - 1) // per_trip


def last_trip(name, shape):
    """a two-quad kernel's last trip: (threads in it, of these with q1 live, with q1 dead -- q1c clamped to q0)"""
    assert name in TWO_QUADS
    st, n = stride(name, shape), items(name, shape)
    start = 2 * st * (trips(name, shape) - 1)
    threads = min(st, n - start)
    live = max(0, min(st, n - start - st))
    return threads, live, threads - live


def threshold(name, shape, arm):
    """the number of loop items above which `arm` is reached at this launch's stride"""
    st = stride(name, shape)
    if name in TWO_QUADS:
        return {'trip 2, q1 live and dead': 3 * st, 'trip 2, q1 dead': 2 * st}[arm]
    return st


def arm(name, shape):
    """the arm a shape reaches, from the arithmetic above"""
    t = trips(name, shape)
    if name in TWO_QUADS:
        if t < 2:
            return 'trip 1'
        _, live, dead = last_trip(name, shape)
        return 'trip %d, %s' % (t, 'q1 live and dead' if live and dead else ('q1 live' if live else 'q1 dead'))
    return 'trip %d' % t


# ------------------------------------------------------------------------------------------------ the cases
OPT_ALIGNED = dict(n=3 + 4 * (3 * T + 300) + 2, offs=(1, 1, 1, 1))      # one element into the allocation: head 3, tail 2
OPT_MIXED = (0, 1, 2, 3)                                               # pairwise different: no common quad grid (adamw uses all four)
ADAM2_COUNT = 4 * (3 * T + 300)
ADAM_TAIL_COUNT = 4 * (T + 300) + 3
GLU_M, GLU_R = 16400, 64                                               # M R = T4 + 1024
FUSED_M = 65600                                                        # M (R / 4) = T4 + 1024

# (id, launcher name, shape, arm claimed, test that runs it).  arm: as arm() spells it; rows of the scalar loops add 'scalar ...'.
CASES = [
    ('adam2', 'adam2_kernel', dict(count=ADAM2_COUNT), 'trip 2, q1 live and dead', 'test_grid_wrap_gpu.py::test_adam_wraps'),
    ('adam tail', 'adam_kernel', dict(count=ADAM_TAIL_COUNT), 'trip 2', 'test_grid_wrap_gpu.py::test_adam_wraps'),
    ('optim quads', 'optim_kernel', OPT_ALIGNED, 'trip 2, q1 live and dead', 'test_grid_wrap_gpu.py::test_optim_wraps'),
    ('optim scalar wrap', 'optim_kernel scalars', dict(n=T + 300, offs=OPT_MIXED), 'trip 2', 'test_grid_wrap_gpu.py::test_optim_wraps'),
    ('relu_mask_bwd', 'relu_mask_bwd', dict(count=T + 300), 'trip 2', 'test_grid_wrap_gpu.py::test_relu_jacobians_wrap'),
    ('relu_scale_bwd', 'relu_scale_bwd', dict(count=4 * (T + 300)), 'trip 2', 'test_grid_wrap_gpu.py::test_relu_jacobians_wrap'),
    ('dropout_mask', 'dropout_mask', dict(count=4 * (T + 300) + 3), 'trip 2', 'test_grid_wrap_gpu.py::test_dropout_masks_wrap'),
    ('dropout_masks', 'dropout_masks', dict(counts=(43, 4 * (T + 300) + 3, 4096)), 'trip 2', 'test_grid_wrap_gpu.py::test_dropout_masks_wrap'),
    ('glu_fwd', 'glu_fwd', dict(M=GLU_M, R=GLU_R), 'trip 2', 'test_grid_wrap_gpu.py::test_glu_family_wraps'),
    ('glu_bwd', 'glu_bwd', dict(M=GLU_M, R=GLU_R), 'trip 2', 'test_grid_wrap_gpu.py::test_glu_family_wraps'),
    ('split_halves', 'split_halves', dict(M=GLU_M // 2, R=GLU_R), 'trip 2', 'test_grid_wrap_gpu.py::test_glu_family_wraps'),
    ('relu_bwd_add', 'relu_bwd_add', dict(M=GLU_M, R=GLU_R), 'trip 2', 'test_grid_wrap_gpu.py::test_glu_family_wraps'),
    ('glu_fwd_fused', 'glu_fwd_fused', dict(M=FUSED_M, R=GLU_R), 'trip 2', 'test_grid_wrap_gpu.py::test_fused_forwards_wrap'),
    ('ctx_fwd_fused', 'ctx_fwd_fused', dict(M=FUSED_M, R=GLU_R), 'trip 2', 'test_grid_wrap_gpu.py::test_fused_forwards_wrap'),
    ('embed_pe_fwd', 'embed_pe_fwd', dict(N=4100, T=4, D=64), 'trip 2', 'test_grid_wrap_gpu.py::test_embed_pe_fwd_wraps'),
    ('meanpool_bwd', 'meanpool_bwd', dict(B=4100, K=4, D=64), 'trip 2', 'test_grid_wrap_gpu.py::test_meanpool_bwd_wraps'),
    # the grid-stride kernel is the atomicAdd arm; 16 400 positions are past EBD_MAX_ROWS, so D = 64 takes it
    ('embed_pe_bwd', 'embed_pe_bwd', dict(N=4100, T=4, D=64), 'trip 2', 'test_grid_wrap_gpu.py::test_embed_pe_bwd_wraps'),
    ('rows_narrow', 'rows_narrow', dict(count=8 * (T + 300) + 3, dst_off=0), 'trip 2', 'test_grid_wrap_gpu.py::test_rows_narrow_wraps'),
    ('rows_narrow head', 'rows_narrow', dict(count=7 + 8 * (T + 300) + 3, dst_off=1), 'trip 2', 'test_grid_wrap_gpu.py::test_rows_narrow_wraps'),
    # already past the threshold in a test the suite has: named here, nothing added
    ('bn_apply', 'bn_apply', dict(rows=1056, D=2048), 'trip 2', 'test_region_norm_arms_gpu.py::test_second_grid_stride_trip'),
    ('bn_apply dword', 'bn_apply', dict(rows=1040, D=2053), 'trip 2', 'test_region_norm_arms_gpu.py::test_second_grid_stride_trip'),
    ('bn_bwd_dx', 'bn_bwd_dx', dict(rows=1056, D=2048), 'trip 2', 'test_region_norm_arms_gpu.py::test_second_grid_stride_trip'),
    ('bn_bwd_dx dword', 'bn_bwd_dx', dict(rows=1040, D=2053), 'trip 2', 'test_region_norm_arms_gpu.py::test_second_grid_stride_trip'),
    ('ema', 'ema_kernel', dict(n=2048 * 256 * 8 + 5, offs=(0, 0)), 'trip 2, q1 dead', 'test_ema_gpu.py (its WRAP count)'),
    # GATHER_CASES rows (24, 50, 50, 1024, 1024) and (20, 50, 50, 1001, None) of test_beam_train_full_gpu.py
    ('lineage_gather float4', 'lineage_gather float4', dict(L=24, rows_dst=50, Ca=1024, Cb=1024), 'trip 2',
     'test_beam_train_full_gpu.py::test_lineage_gather_vs_torch'),
    ('lineage_gather float', 'lineage_gather float', dict(L=20, rows_dst=50, Ca=1001, Cb=0), 'trip 2',
     'test_beam_train_full_gpu.py::test_lineage_gather_vs_torch'),
]
# rows of tests from before this table: their shapes were not chosen against MINIMAL
EXISTING = ('bn_apply', 'bn_apply dword', 'bn_bwd_dx', 'bn_bwd_dx dword', 'ema', 'lineage_gather float4', 'lineage_gather float')

# capmi_optim_step, scalar throughout (the buffers' misalignments differ) with a single trip of the scalar loop: (n, offsets)
OPTIM_SCALAR_SINGLE = [(1, OPT_MIXED), (5, OPT_MIXED), (1023, OPT_MIXED)]


def case(cid):
    return next(c for c in CASES if c[0] == cid)


def shape_of(cid):
    return case(cid)[2]


# ------------------------------------------------------------------------------------------------ the sources
def grid_for_calls(fname):
    """(the line, the argument text) of every grid_for( call in a source file; the definition in host_common.h is no call"""
    out = []
    with open(os.path.join(CSRC, fname)) as f:
        for line in f:
            for m in re.finditer(r'grid_for\(', line):
                depth, i = 1, m.end()
                while i < len(line) and depth:
                    depth += {'(': 1, ')': -1}.get(line[i], 0)
                    i += 1
                if depth == 0:
                    out.append((line, line[m.end():i - 1]))
    return out


def source_args(name):
    """the argument texts of the grid_for( calls that launch `name`'s kernel"""
    fname, kernel, _, _, _, _ = LAUNCHERS[name]
    return [a for line, a in grid_for_calls(fname) if (kernel is None and 'hipLaunchKernelGGL' not in line) or (kernel and kernel in line)]
