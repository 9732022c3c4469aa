#!/usr/bin/env python
"""Generates ``tests/golden/balanced_sampler_golden.npz`` by EXECUTING THE REFERENCE's Libra R-CNN samplers on the CPU:
``CombinedSampler`` (mmdet/core/bbox/samplers/combined_sampler.py:5-16) over ``InstanceBalancedPosSampler``
(instance_balanced_pos_sampler.py:9-41), ``IoUBalancedNegSampler`` (iou_balanced_neg_sampler.py:44-133) and
``RandomSampler`` (random_sampler.py:35-53), through ``BaseSampler.sample`` (base_sampler.py:31-78) with
``add_gt_as_proposals``, so ``AssignResult.add_gt_`` (assign_result.py) runs too.  Imported through oracle/ref_import.

Run where the reference tree is present:

    python tests/golden/make_golden_balanced_sampler.py

What is stood in for:

* ``np.int`` (iou_balanced_neg_sampler.py:62,116,122), which the numpy this was generated with no longer has: the
  builtin ``int``, which is what the alias was;
* ``set`` inside instance_balanced_pos_sampler.py (line 33: ``set(pos_inds.cpu()) - set(sampled_inds.cpu())``): a set of
  the index VALUES.  The reference's sets hold 0-d tensors, which hash by identity, so its difference removes nothing
  and its fill draws from all positives, duplicates included, which the later ``unique()`` drops: fewer than
  ``num_expected`` positives come back, by a random amount.  The contract of ``bgs_sample_rois_balanced`` is the fill
  from the REMAINING positives; with the set over values the reference's own lines compute it.

What is observed (pure recorders, every return value is the reference's own):

* ``_sample_pos`` / ``_sample_neg``: their ``num_expected`` arguments (``n_exp_pos``, ``n_exp_neg``);
* ``round`` inside instance_balanced_pos_sampler.py:18: its result, so ``num_per_gt`` = result + 1;
* ``sample_via_interval``: its ``num_expected`` (``n_iou_exp``);
* ``RandomSampler.random_choice``: ``(len(gallery), num)`` of every call, in order (``ref_choices``).  A case without
  a call has no random choice left: its sampled sets are THE answer.

Recorded per case ``k``: the inputs after ``add_gt_`` (``c{k}_assigned`` int16, ``c{k}_max_overlaps`` float32,
``c{k}_n_gt``), the parameters (``c{k}_params``, balanced_sampler_ref.PARAM_NAMES), ``c{k}_ref_ints`` = (n_exp_pos,
n_exp_neg, num_per_gt or -1, n_iou_exp or -1, #pos returned, #neg returned), ``c{k}_ref_choices`` [K, 2],
``c{k}_ref_pos`` / ``c{k}_ref_neg``: the sorted indices the reference returned for its numpy draw.
"""
import builtins
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import balanced_sampler_ref as R    # noqa: E402

OUT = os.path.join(HERE, 'balanced_sampler_golden.npz')
SEED = 20261


def _proposals(rs, n, n_gt, pos_rate, ignore_rate=0.03, neg_hi=0.5, owner=None, gt_weights=None):
    """Assignment and overlaps of ``n`` proposals: negatives with overlaps in [0, neg_hi) (a tenth exactly 0),
    positives of gt 1..n_gt (``owner``: all of one gt; ``gt_weights``: relative shares) in [0.5, 1), a few ignored."""
    a = np.zeros(n, np.int64)
    mo = (rs.rand(n) * neg_hi).astype(np.float32)
    mo[rs.rand(n) < 0.1] = 0.0
    pos = rs.rand(n) < pos_rate
    w = np.ones(n_gt) if gt_weights is None else np.asarray(gt_weights, float)
    a[pos] = owner if owner is not None else rs.choice(n_gt, size=int(pos.sum()), p=w / w.sum()) + 1
    mo[pos] = (0.5 + 0.5 * rs.rand(int(pos.sum()))).astype(np.float32)
    ign = (rs.rand(n) < ignore_rate) & ~pos
    a[ign] = -1
    return a, mo


def cases():
    """-> list of (name, proposals' gt_inds, proposals' max_overlaps, n_gt, params).  Candidates = n_gt + proposals."""
    rs = np.random.RandomState(SEED)
    out = []

    def add(name, a, mo, n_gt, num, pos_fraction=0.25, neg_pos_ub=-1, pos_mode=1, neg_mode=1, floor_thr=-1,
            floor_fraction=0, num_bins=3):
        out.append((name, a, mo, n_gt, dict(num=num, pos_fraction=pos_fraction, neg_pos_ub=neg_pos_ub,
                                            pos_mode=pos_mode, neg_mode=neg_mode, floor_thr=floor_thr,
                                            floor_fraction=floor_fraction, num_bins=num_bins)))

    add('a0_3gt_only', np.zeros(0, np.int64), np.zeros(0, np.float32), 3, 16)
    a, mo = _proposals(rs, 36, 1, 0.5, owner=1)
    add('a37_one_gt_owns_all', a, mo, 1, 16)
    a, mo = _proposals(rs, 34, 3, 0.2)
    add('a37_all_under_quota', a, mo, 3, 64, floor_thr=0.1, floor_fraction=0.3)
    a, mo = _proposals(rs, 297, 3, 0.3)
    add('a300_g3_thr0_cut', a, mo, 3, 64, floor_thr=0, floor_fraction=0.3)
    a, mo = _proposals(rs, 297, 3, 0.3, gt_weights=[0.01, 1, 1])
    add('a300_g3_fill', a, mo, 3, 64, floor_thr=0.1, floor_fraction=0.3, num_bins=2)
    a, mo = _proposals(rs, 283, 17, 0.1)
    add('a300_g17_ub3', a, mo, 17, 64, neg_pos_ub=3, floor_thr=0.1, floor_fraction=0.3, num_bins=2)
    a, mo = _proposals(rs, 283, 17, 0.4)
    add('a300_g17_num16', a, mo, 17, 16, floor_thr=0.1, floor_fraction=0)
    a, mo = _proposals(rs, 240, 60, 0.2)
    add('a300_g60_num512_all', a, mo, 60, 512, floor_thr=0, floor_fraction=0.3)
    # the middle interval [0.4, 0.7) of [0.1, 1.0) empty as well as the last
    a, mo = _proposals(rs, 297, 3, 0.05, neg_hi=0.4)
    add('a300_empty_intervals', a, mo, 3, 64, floor_thr=0.1, floor_fraction=0.3)
    # overlaps exactly on the float32 interval bounds (and one ulp either side), negatives up to 0.8
    a, mo = _proposals(rs, 297, 3, 0.05, neg_hi=0.8)
    neg = np.nonzero(a == 0)[0]
    itv = (np.float32(1.0) - 0.1) / 3
    bounds = [np.float32(0.1), 0.1 + 1 * itv, 0.1 + 2 * itv]
    vals = []
    for b in bounds:
        vals += [b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(1))]
    for j, v in enumerate(vals * 4):
        mo[neg[j]] = v
    add('a300_on_bounds_thr01', a, mo, 3, 64, floor_thr=0.1, floor_fraction=0.3)
    a, mo = a.copy(), mo.copy()
    for j, v in enumerate([np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(0)), np.float32(0.0)] * 6):
        mo[neg[j]] = v
    add('a300_on_bounds_thr0_bins2', a, mo, 3, 64, floor_thr=0, floor_fraction=0, num_bins=2)
    a, mo = _proposals(rs, 4036, 60, 0.1)
    add('a4096_g60_libra', a, mo, 60, 512)
    a, mo = _proposals(rs, 4036, 60, 0.1)
    add('a4096_g60_round_half_even', a, mo, 60, 64, pos_fraction=0.46875)
    a, mo = _proposals(rs, 4079, 17, 0.01)
    add('a4096_g17_few_pos', a, mo, 17, 512, floor_thr=0.1, floor_fraction=0.3)
    a, mo = _proposals(rs, 4093, 3, 0.05)
    add('a4096_g3_bins1', a, mo, 3, 64, floor_thr=0, floor_fraction=0.3, num_bins=1)
    a, mo = _proposals(rs, 4095, 1, 0.005, owner=1)
    add('a4096_g1_ub3', a, mo, 1, 512, neg_pos_ub=3, floor_thr=0.1, floor_fraction=0.3)
    # few negatives in the IoU set: all of it taken, the floor set and the final fill make up the rest
    a, mo = _proposals(rs, 297, 3, 0.05, neg_hi=0.12)
    add('a300_iou_set_short', a, mo, 3, 64, floor_thr=0.1, floor_fraction=0.3)
    a, mo = _proposals(rs, 297, 3, 0.05)
    mo[(a == 0) & (np.arange(297) % 7 > 0)] = -0.25     # in neither set (no assigner emits it): the final fill's ground
    add('a300_neither_set', a, mo, 3, 64, floor_thr=0.1, floor_fraction=0.3)
    # floor_thr = 0: the floor set is the exact zeros; five of them, under its share, so the final fill runs
    a, mo = _proposals(rs, 297, 3, 0.3)
    zero = np.nonzero((a == 0) & (mo == 0))[0]
    mo[zero[5:]] = np.float32(0.01)
    add('a300_floor_short_final_fill', a, mo, 3, 64, floor_thr=0, floor_fraction=0.3)
    # floor_thr = -1 with a floor share: the floor set is empty, so that share comes from the final fill
    a, mo = _proposals(rs, 299, 1, 0.2, owner=1)
    add('a300_g1_thr_neg1_floor_share', a, mo, 1, 64, floor_thr=-1, floor_fraction=0.3)
    a, mo = _proposals(rs, 283, 17, 0.4)
    add('a300_pos_random_neg_iou', a, mo, 17, 64, pos_mode=0, floor_thr=0, floor_fraction=0.3)
    a, mo = _proposals(rs, 283, 17, 0.4)
    add('a300_pos_instance_neg_random', a, mo, 17, 64, neg_mode=0)
    a, mo = _proposals(rs, 283, 17, 0.4)
    add('a300_both_random', a, mo, 17, 64, pos_mode=0, neg_mode=0, neg_pos_ub=3)
    return out


POS_TYPES = {0: 'RandomSampler', 1: 'InstanceBalancedPosSampler'}
NEG_TYPES = {0: 'RandomSampler', 1: 'IoUBalancedNegSampler'}


def run_reference(a, mo, n_gt, par, log):
    from mmdet.core.bbox.samplers.combined_sampler import CombinedSampler
    from mmdet.core.bbox.assigners.assign_result import AssignResult
    neg_cfg = dict(type=NEG_TYPES[par['neg_mode']])
    if par['neg_mode'] == 1:
        neg_cfg.update(floor_thr=par['floor_thr'], floor_fraction=par['floor_fraction'], num_bins=par['num_bins'])
    sampler = CombinedSampler(num=par['num'], pos_fraction=par['pos_fraction'], neg_pos_ub=par['neg_pos_ub'],
                              add_gt_as_proposals=True, pos_sampler=dict(type=POS_TYPES[par['pos_mode']]),
                              neg_sampler=neg_cfg)
    for who, name in ((sampler.pos_sampler, '_sample_pos'), (sampler.neg_sampler, '_sample_neg')):
        def rec(assign_result, num_expected, _f=getattr(who, name), _n=name, **kw):
            log[_n] = int(num_expected)
            return _f(assign_result, num_expected, **kw)
        setattr(who, name, rec)
    if par['neg_mode'] == 1:
        via = sampler.neg_sampler.sample_via_interval

        def via_rec(max_overlaps, full_set, num_expected):
            log['via'] = int(num_expected)
            return via(max_overlaps, full_set, num_expected)
        sampler.neg_sampler.sample_via_interval = via_rec
    ar = AssignResult(n_gt, torch.from_numpy(a), torch.from_numpy(mo), labels=torch.zeros(len(a), dtype=torch.long))
    res = sampler.sample(ar, torch.zeros(len(a), 4), torch.zeros(n_gt, 4), torch.arange(1, n_gt + 1))
    return ar, res


def main():
    from oracle import ref_import
    ref_import.install_stubs()
    np.int = int
    import mmdet.core.bbox.samplers.instance_balanced_pos_sampler as IB
    from mmdet.core.bbox.samplers.random_sampler import RandomSampler
    log = {}
    IB.set = lambda it: builtins.set(int(x) for x in it)

    def round_rec(x):
        log['round'] = round(x)
        return log['round']
    IB.round = round_rec
    choice = RandomSampler.random_choice

    def choice_rec(gallery, num):
        log['choices'].append((len(gallery), int(num)))
        return choice(gallery, num)
    RandomSampler.random_choice = staticmethod(choice_rec)

    np.random.seed(SEED)                         # the reference draws with the global numpy RNG
    rec, names = {}, []
    for k, (name, a, mo, n_gt, par) in enumerate(cases()):
        log.clear()
        log['choices'] = []
        ar, res = run_reference(a, mo, n_gt, par, log)
        p = 'c%d_' % k
        names.append(name)
        full_a, full_mo = ar.gt_inds.numpy(), ar.max_overlaps.numpy()
        assert len(full_a) == n_gt + len(a) and (full_mo[:n_gt] == 1).all()
        rec[p + 'assigned'] = full_a.astype(np.int16)
        rec[p + 'max_overlaps'] = full_mo.astype(np.float32)
        rec[p + 'n_gt'] = np.int64(n_gt)
        rec[p + 'params'] = np.array([par[n] for n in R.PARAM_NAMES], np.float64)
        pos, neg = res.pos_inds.numpy(), res.neg_inds.numpy()
        rec[p + 'ref_ints'] = np.array([log['_sample_pos'], log['_sample_neg'], log.get('round', -2) + 1,
                                        log.get('via', -1), len(pos), len(neg)], np.int64)
        rec[p + 'ref_choices'] = np.array(log['choices'], np.int64).reshape(-1, 2)
        rec[p + 'ref_pos'] = pos.astype(np.int32)
        rec[p + 'ref_neg'] = neg.astype(np.int32)
        q = R.quotas(full_a, full_mo, **par)
        print('%-30s A=%4d pos %4d neg %4d | n_exp %3d/%3d per_gt %3d iou_exp %3d | returned %3d + %3d | %-6s %-8s '
              'fill %3d | %d choices%s' % (name, len(full_a), q['n_pos'], q['n_neg'], log['_sample_pos'],
                                           log['_sample_neg'], log.get('round', -2) + 1, log.get('via', -1), len(pos),
                                           len(neg), q['pos_case'], q['neg_case'], q['n_fill'], len(log['choices']),
                                           '' if log['choices'] else '  DETERMINISTIC'))
    rec['names'] = np.array(names)
    np.savez_compressed(OUT, **rec)
    print('wrote %s (%.1f KB)' % (OUT, os.path.getsize(OUT) / 1024.0))


if __name__ == '__main__':
    main()
