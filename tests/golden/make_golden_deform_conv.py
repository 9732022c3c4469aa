#!/usr/bin/env python
"""Regenerates tests/golden/deform_conv_golden.npz by EXECUTING the reference's deformable-conv kernels.

    python tests/golden/make_golden_deform_conv.py        (needs the reference tree: BGS_REFERENCE_ROOT)

The three ``__global__`` templates of mmdet/ops/dcn/src/deform_conv_cuda_kernel.cu — ``deformable_im2col_gpu_kernel``,
``deformable_col2im_gpu_kernel``, ``deformable_col2im_coord_gpu_kernel`` — and their ``__device__`` helpers are plain
C++ once ``__global__`` / ``__device__`` / ``blockIdx`` ... / ``atomicAdd`` have host meanings (the file's own
``CUDA_KERNEL_LOOP`` then runs as a serial loop).  This script reads those function bodies FROM THE REFERENCE FILE WHERE IT
LIES (the ATen launchers between them need nvcc and are left out), writes the translation unit into a temporary directory,
compiles it with ``g++ -O2`` and calls it through ctypes; nothing of it is kept.  The host glue of deform_conv_cuda.cpp
(per-group ``addmm``, views) needs ATen-CUDA: it is restated in float64 numpy (tests/deform_conv_ref.py).

Per case (tests/deform_conv_ref.py:CASES; inputs are regenerated from their seeds by ``case_inputs`` and pinned here by
digest, offsets included, so that the file stays small) the fixture holds, computed with the reference kernels for sampling
and scatter and float64 for the GEMMs:
  ``col``  the reference's columns (bit-exact float32) of the channels ``col_channels`` = (0, C - 1): with one deformable
           group the sampling is the same function of every channel's plane, so two channels pin all of its arithmetic;
  ``y`` / ``dx`` / ``dw``  the channels of the LAST group (a grouped conv's groups are independent); ``doffset`` in full
           (it sums over every channel).
Every case samples exactly at -1, 0, H - 1, H (W likewise) and one ulp below and above each, on both axes (asserted here and
in tests/test_deform_conv_cpu.py).  A forward-only case plants NaN / +-inf / +-1e30 offsets.  The block case executes the reference's own ResNeXt
``Bottleneck`` with ``dcn`` on the CPU (``mmdet.ops.dcn.deform_conv.deform_conv`` rebound to the compiled im2col: the
reference's Function raises on CPU tensors) and records input, parameters, output and the state-dict names / shapes.
"""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.ref_import import REFERENCE_ROOT as REF  # noqa: E402  (BGS_REFERENCE_ROOT)
from tests import deform_conv_ref as R  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'deform_conv_golden.npz')

_SHIM = r"""
// GENERATED from %(src)s -- build output, not source.
#include <algorithm>
#include <cmath>
using std::abs;
using std::floor;
#define __device__
#define __global__
struct BgsDim3 { int x, y, z; };
static BgsDim3 blockIdx = {0, 0, 0}, blockDim = {1, 1, 1}, threadIdx = {0, 0, 0}, gridDim = {1, 1, 1};
template <typename T> static inline void atomicAdd(T* p, T v) { *p += v; }
%(loop)s
%(body)s
extern "C" void ref_im2col(int n, const float* im, const float* off, int H, int W, int s, int N, int C, int Ho, int Wo,
                           float* col) {
  deformable_im2col_gpu_kernel<float>(n, im, off, H, W, 3, 3, 1, 1, s, s, 1, 1, C, N, C, 1, Ho, Wo, col);
}
extern "C" void ref_col2im(int n, const float* col, const float* off, int C, int H, int W, int s, int N, int Ho, int Wo,
                           float* grad_im) {
  deformable_col2im_gpu_kernel<float>(n, col, off, C, H, W, 3, 3, 1, 1, s, s, 1, 1, C, N, 1, Ho, Wo, grad_im);
}
extern "C" void ref_col2im_coord(int n, const float* col, const float* im, const float* off, int C, int H, int W, int s,
                                 int N, int Ho, int Wo, float* grad_off) {
  deformable_col2im_coord_gpu_kernel<float>(n, col, im, off, C, H, W, 3, 3, 1, 1, s, s, 1, 1, C * 9, N, 18, 1, Ho, Wo,
                                            grad_off);
}
"""


def build_reference_kernels(tmp):
    src = os.path.join(REF, 'mmdet/ops/dcn/src/deform_conv_cuda_kernel.cu')
    lines = open(src).read().split('\n')
    lo = next(i for i, l in enumerate(lines) if l.startswith('#define CUDA_KERNEL_LOOP'))
    loop = '\n'.join(lines[lo:lo + 3])
    start = next(i for i, l in enumerate(lines) if 'deformable_im2col_bilinear' in l) - 1
    end = next(i for i, l in enumerate(lines) if 'dmcn_im2col_bilinear' in l) - 1
    body = '\n'.join(lines[start:end])
    # the ATen launchers (void deformable_*(... at::Tensor ...) { ... }) are left out
    body = re.sub(r'\nvoid deformable_\w+\([^)]*\)\n\{.*?\n\}\n', '\n', body, flags=re.S)
    assert 'at::' not in body and body.count('__global__') == 3, 'unexpected reference text'
    cpp, so = os.path.join(tmp, 'dcn_ref.cpp'), os.path.join(tmp, 'dcn_ref.so')
    with open(cpp, 'w') as f:
        f.write(_SHIM % dict(src=src, loop=loop, body=body))
    subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-o', so, cpp])
    lib = ctypes.CDLL(so)
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.ref_im2col.argtypes = [i, p, p] + [i] * 7 + [p]
    lib.ref_col2im.argtypes = [i, p, p] + [i] * 7 + [p]
    lib.ref_col2im_coord.argtypes = [i, p, p, p] + [i] * 7 + [p]
    for f in (lib.ref_im2col, lib.ref_col2im, lib.ref_col2im_coord):
        f.restype = None
    return lib


def _nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)), dtype=np.float32)


def ref_columns(lib, x, offset, stride):
    """x [N,H,W,C], offset [N,Ho,Wo,18] -> the reference's columns as [N,Ho,Wo,9,C] float32."""
    N, H, W, C = x.shape
    Ho, Wo = R.out_size(H, W, stride)
    im, off = _nchw(x), _nchw(offset)
    col = np.zeros((C * 9, N, Ho, Wo), dtype=np.float32)
    lib.ref_im2col(C * N * Ho * Wo, im.ctypes.data, off.ctypes.data, H, W, stride, N, C, Ho, Wo, col.ctypes.data)
    return np.ascontiguousarray(col.reshape(C, 9, N, Ho, Wo).transpose(2, 3, 4, 1, 0))


def _col_layout(dcol):
    """[N,Ho,Wo,9,C] -> the reference's [C*9, N, Ho, Wo] float32."""
    N, Ho, Wo, _, C = dcol.shape
    return np.ascontiguousarray(dcol.transpose(4, 3, 0, 1, 2).reshape(C * 9, N, Ho, Wo), dtype=np.float32)


def ref_backward_input(lib, x, offset, dcol, stride):
    N, H, W, C = x.shape
    Ho, Wo = R.out_size(H, W, stride)
    im, off, col = _nchw(x), _nchw(offset), _col_layout(dcol)
    gim = np.zeros((N, C, H, W), dtype=np.float32)
    lib.ref_col2im(C * 9 * N * Ho * Wo, col.ctypes.data, off.ctypes.data, C, H, W, stride, N, Ho, Wo, gim.ctypes.data)
    goff = np.zeros((N, 18, Ho, Wo), dtype=np.float32)
    lib.ref_col2im_coord(N * 18 * Ho * Wo, col.ctypes.data, im.ctypes.data, off.ctypes.data, C, H, W, stride, N, Ho, Wo,
                         goff.ctypes.data)
    return gim.transpose(0, 2, 3, 1), goff.transpose(0, 2, 3, 1)


def make_case(lib, case, out, forward_only=False):
    name, cg, stride, (H, W) = case
    inp = R.case_inputs(case)
    x, offset, w, dz = inp['x'], inp['offset'], inp['w'], inp['dz']
    C = cg * R.GROUPS
    last = slice(C - cg, C)
    col = ref_columns(lib, x, offset, stride)
    assert np.isfinite(col).all()
    y = R.forward_from_columns(col, w, None, R.GROUPS)
    out[name + '/digest'] = np.array(R.digest(x, offset, w, dz))
    missing = R.named_values_present(offset, H, W, stride)
    assert not missing, 'case %s lacks the boundary samples %s' % (name, missing)
    out[name + '/col_channels'] = np.array([0, C - 1])
    out[name + '/col'] = np.ascontiguousarray(col[..., [0, C - 1]])
    out[name + '/y_last_group'] = y[..., last].astype(np.float32)
    geo = R.geometry(offset, H, W, stride)
    stats = dict(inside=int(geo['inside'].sum()), taps=int(geo['inside'].size),
                 integer=int(((geo['h'] == np.floor(geo['h'])) & geo['inside']).sum()),
                 edge=int((geo['inside'] & ((geo['h'] < 0) | (geo['h'] > H - 1) | (geo['w'] < 0) | (geo['w'] > W - 1))).sum()))
    print(name, stats, 'restatement == executed columns:', np.array_equal(R.columns(x, offset, stride), col))
    if forward_only:
        return
    dcol = R.dcolumns(w, dz, R.GROUPS)                                   # float64 GEMM
    dx, doff = ref_backward_input(lib, x, offset, dcol, stride)          # reference scatter / coordinate kernels
    dzg = dz.astype(np.float64).reshape(R.BATCH, -1, R.GROUPS, cg)
    Ho, Wo = R.out_size(H, W, stride)
    dw = np.einsum('nmgo,nmtgl->gotl', dzg, col.astype(np.float64).reshape(R.BATCH, Ho * Wo, 9, R.GROUPS, cg))
    out[name + '/dx_last_group'] = np.ascontiguousarray(dx[..., last], dtype=np.float32)
    out[name + '/doffset'] = np.ascontiguousarray(doff, dtype=np.float32)
    out[name + '/dw_last_group'] = dw[-1].astype(np.float32)            # [cg, 9, cg] of the last group
    dx64, doff64, dw64, _ = R.backward(x, offset, w, dz, R.GROUPS, stride)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())     # noqa: E731
    print('   executed vs float64 restatement: dx %.2e doffset %.2e dw %.2e' %
          (rel(dx, dx64), rel(doff, doff64), rel(dw.reshape(C, 3, 3, cg), dw64)))


def make_block_case(lib, out):
    """The reference's ResNeXt Bottleneck with dcn, executed on the CPU."""
    import torch
    from oracle import ref_import
    ref_import.install_stubs()
    from mmdet.models.backbones.resnext import Bottleneck
    ref_dc = sys.modules['mmdet.ops.dcn.deform_conv']     # (the package attribute of that name is the function)

    def deform_conv_cpu(x, offset, weight, stride, padding, dilation, groups, deformable_groups):
        assert tuple(padding) == (1, 1) and tuple(dilation) == (1, 1) and deformable_groups == 1
        s = stride[0]
        xn = x.detach().numpy().transpose(0, 2, 3, 1)
        on = offset.detach().numpy().transpose(0, 2, 3, 1)
        col = ref_columns(lib, np.ascontiguousarray(xn), np.ascontiguousarray(on), s)
        wn = weight.detach().numpy().transpose(0, 2, 3, 1)
        y = R.forward_from_columns(col, wn, None, groups)
        return torch.from_numpy(y.astype(np.float32).transpose(0, 3, 1, 2).copy())

    ref_dc.deform_conv = deform_conv_cpu
    torch.manual_seed(20)
    inplanes, planes, groups, base_width, stride = 16, 32, 8, 8, 2
    dcn = dict(modulated=False, groups=groups, deformable_groups=1, fallback_on_stride=False)
    ds = torch.nn.Sequential(torch.nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False),
                             torch.nn.BatchNorm2d(planes * 4))
    blk = Bottleneck(inplanes, planes, groups=groups, base_width=base_width, stride=stride, downsample=ds, dcn=dcn)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
        blk.conv2_offset.weight.normal_(0, 0.05)
        blk.conv2_offset.bias.normal_(0, 1.0)
    blk.eval()
    x = torch.randn(2, inplanes, 9, 11)
    with torch.no_grad():
        y = blk(x)
    sd = blk.state_dict()
    out['block/cfg'] = np.array([inplanes, planes, groups, base_width, stride])
    out['block/x'] = x.numpy()
    out['block/y'] = y.numpy()
    out['block/names'] = np.array(sorted(sd.keys()))
    for k, v in sd.items():
        out['block/param/' + k] = v.numpy()
    print('block', tuple(x.shape), '->', tuple(y.shape), len(sd), 'state-dict entries')


def main():
    if not os.path.isdir(REF):
        sys.exit('reference tree not found at %s' % REF)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_reference_kernels(tmp)
        # the recipe's own check: at zero offsets the compiled im2col is F.unfold exactly
        import torch
        x = np.random.RandomState(0).standard_normal((2, 7, 6, 4)).astype(np.float32)
        col = ref_columns(lib, x, np.zeros((2, 7, 6, 18), np.float32), 1)
        unf = torch.nn.functional.unfold(torch.from_numpy(_nchw(x)), 3, padding=1).view(2, 4, 9, 7, 6)
        assert np.array_equal(col, unf.permute(0, 3, 4, 2, 1).numpy())
        for case in R.CASES:
            make_case(lib, case, out)
        make_case(lib, R.NONFINITE_CASE, out, forward_only=True)
        make_block_case(lib, out)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
