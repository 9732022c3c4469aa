"""Plain-numpy restatement of the quota arithmetic of the Libra R-CNN samplers, for the balanced-sampler tests.

``quotas()`` restates, for one image, every integer that ``BaseSampler.sample`` (base_sampler.py:60-75),
``InstanceBalancedPosSampler._sample_pos`` (instance_balanced_pos_sampler.py:9-41) and
``IoUBalancedNegSampler._sample_neg`` / ``sample_via_interval`` (iou_balanced_neg_sampler.py:44-133) compute on the way
to their draws, and the sequence of ``random_choice(gallery, num)`` calls they make, as ``(len(gallery), num)`` pairs.
tests/test_balanced_sampler_cpu.py pins it to the integers and the call sequence RECORDED from the executed reference
(tests/golden/balanced_sampler_golden.npz); tests/test_gpu_balanced_sampler.py then holds the kernel's draws to it
through ``check_sample()``, which the CPU test also runs over the reference's own recorded draw.

One deviation from the reference is part of the contract: the positives' fill draws from the REMAINING
positives, so exactly ``min(#pos, int(num * pos_fraction))`` positives are returned.  The fixture was recorded with
that one line of the reference evaluated over index values instead of tensor identities.
"""
import numpy as np

PARAM_NAMES = ('num', 'pos_fraction', 'neg_pos_ub', 'pos_mode', 'neg_mode', 'floor_thr', 'floor_fraction', 'num_bins')


def load_cases(path):
    """-> list of dicts: name, assigned int32 [A], max_overlaps float32 [A] (both AFTER add_gt_), n_gt, the sampler
    parameters, and the recorded reference answers (``ref_*``)."""
    z = np.load(path, allow_pickle=False)
    cases = []
    for k, name in enumerate(z['names']):
        p = 'c%d_' % k
        par = z[p + 'params']
        c = dict(name=str(name), assigned=z[p + 'assigned'].astype(np.int32), max_overlaps=z[p + 'max_overlaps'],
                 n_gt=int(z[p + 'n_gt']))
        for n, v in zip(PARAM_NAMES, par):
            c[n] = float(v) if n in ('pos_fraction', 'floor_thr', 'floor_fraction') else int(v)
        for key in ('ints', 'choices', 'pos', 'neg'):
            c['ref_' + key] = z[p + 'ref_' + key]
        cases.append(c)
    return cases


def params(c):
    return {n: c[n] for n in PARAM_NAMES}


def neg_sets(max_overlaps, floor_thr):
    """iou_balanced_neg_sampler.py:86-100 -> boolean (floor set, IoU set) over all candidates."""
    mo = max_overlaps
    if floor_thr > 0:
        return np.logical_and(mo >= 0, mo < floor_thr), mo >= floor_thr
    if floor_thr == 0:
        return mo == 0, mo > floor_thr
    return np.zeros(mo.shape, bool), mo > floor_thr


def interval_of(max_overlaps, floor_thr, num_bins):
    """sample_via_interval:45-56 -> the interval index of every candidate, -1 outside all of them.  The bounds are
    float32, as numpy evaluates ``floor_thr + i * iou_interval`` with a float32 ``max_overlaps.max()``."""
    mo = max_overlaps
    max_iou = mo.max()
    iou_interval = (max_iou - floor_thr) / num_bins
    assert isinstance(iou_interval, np.float32)
    out = np.full(mo.shape, -1, np.int64)
    for i in range(num_bins):
        start_iou = floor_thr + i * iou_interval
        end_iou = floor_thr + (i + 1) * iou_interval
        assert isinstance(start_iou, np.float32) and isinstance(end_iou, np.float32)
        m = np.logical_and(mo >= start_iou, mo < end_iou)
        assert (out[m] == -1).all()
        out[m] = i
    return out


def quotas(assigned, max_overlaps, num, pos_fraction, neg_pos_ub=-1, pos_mode=1, neg_mode=1, floor_thr=-1,
           floor_fraction=0, num_bins=3):
    a = np.asarray(assigned)
    mo = np.asarray(max_overlaps, np.float32)
    q = dict(choices=[])
    pos, neg = a > 0, a == 0
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    n_exp = int(num * pos_fraction)
    q.update(n_pos=n_pos, n_neg=n_neg, n_exp_pos=n_exp, k_pos=min(n_pos, n_exp), num_per_gt=-1, pos_case='all',
             gt_ids=np.zeros(0, np.int64), gt_first=np.zeros(0, np.int64))
    # ---- positives
    if n_pos > n_exp:
        if pos_mode == 0:
            q['pos_case'] = 'random'
            q['choices'].append((n_pos, n_exp))
        else:
            ids, cnt = np.unique(a[pos], return_counts=True)
            num_per_gt = int(round(n_exp / float(len(ids))) + 1)
            first = np.minimum(cnt, num_per_gt)
            for c in cnt:
                if c > num_per_gt:
                    q['choices'].append((int(c), num_per_gt))
            u = int(first.sum())
            if u < n_exp:
                q['pos_case'] = 'fill'
                if n_pos - u > n_exp - u:
                    q['choices'].append((n_pos - u, n_exp - u))
            elif u > n_exp:
                q['pos_case'] = 'cut'
                q['choices'].append((u, n_exp))
            else:
                q['pos_case'] = 'exact'
            q.update(num_per_gt=num_per_gt, gt_ids=ids.astype(np.int64), gt_first=first.astype(np.int64))
    # ---- negatives
    n_exp_neg = num - q['k_pos']
    if neg_pos_ub >= 0:
        n_exp_neg = min(n_exp_neg, int(neg_pos_ub * max(1, q['k_pos'])))
    q.update(n_exp_neg=n_exp_neg, k_neg=min(n_neg, n_exp_neg), neg_case='all', n_iou_exp=-1, per_bin=-1,
             bin_first=np.zeros(0, np.int64), iou_min=0, floor_min=0, n_fill=0)
    if n_neg > n_exp_neg:
        if neg_mode == 0:
            q['neg_case'] = 'random'
            q['choices'].append((n_neg, n_exp_neg))
        else:
            q['neg_case'] = 'balanced'
            floor_set, iou_set = neg_sets(mo, floor_thr)
            n_floor, n_iou = int((floor_set & neg).sum()), int((iou_set & neg).sum())
            n_iou_exp = int(n_exp_neg * (1 - floor_fraction))
            q['n_iou_exp'] = n_iou_exp
            if n_iou > n_iou_exp:
                s_iou = n_iou_exp
                if num_bins >= 2:
                    per = int(n_iou_exp / num_bins)
                    itv = interval_of(mo, floor_thr, num_bins)
                    cnt = np.array([int(((itv == i) & iou_set & neg).sum()) for i in range(num_bins)], np.int64)
                    first = np.minimum(cnt, per)
                    for c in cnt:
                        if c > per:
                            q['choices'].append((int(c), per))
                    got = int(first.sum())
                    if got < n_iou_exp:
                        q['choices'].append((n_iou - got, n_iou_exp - got))
                    q.update(per_bin=per, bin_first=first, interval=itv)
                else:
                    q['choices'].append((n_iou, n_iou_exp))
            else:
                s_iou = n_iou
            n_floor_exp = n_exp_neg - s_iou
            if n_floor > n_floor_exp:
                q['choices'].append((n_floor, n_floor_exp))
            s_floor = min(n_floor, n_floor_exp)
            n_fill = n_exp_neg - s_iou - s_floor
            if n_fill > 0:
                q['choices'].append((n_neg - s_iou - s_floor, n_fill))
            q.update(iou_min=s_iou, floor_min=s_floor, n_fill=n_fill, floor_set=floor_set & neg, iou_set=iou_set & neg)
    q['deterministic'] = not q['choices']
    return q


def inclusion_probability(q, assigned):
    """The probability with which each candidate is in the sample when every ``random_choice`` is a uniform subset
    independent of the others: a member of a group of ``n`` with quota ``k`` is drawn with ``k / n``, and one left over
    by an earlier draw joins a later fill of ``e`` out of ``r`` remaining with ``e / r``."""
    a = np.asarray(assigned)
    p = np.zeros(len(a), np.float64)
    pos, neg = a > 0, a == 0
    if q['pos_case'] in ('all', 'random'):
        p[pos] = q['k_pos'] / max(q['n_pos'], 1)
    else:
        u = int(q['gt_first'].sum())
        for g, first in zip(q['gt_ids'], q['gt_first']):
            m = a == g
            p1 = first / m.sum()
            if q['pos_case'] == 'cut':
                p[m] = p1 * q['n_exp_pos'] / u
            elif q['pos_case'] == 'fill':
                p[m] = p1 + (1 - p1) * (q['n_exp_pos'] - u) / (q['n_pos'] - u)
            else:
                p[m] = p1
    if q['neg_case'] in ('all', 'random'):
        p[neg] = q['k_neg'] / max(q['n_neg'], 1)
    else:
        iou, floor = q['iou_set'], q['floor_set']
        n_iou, n_floor = int(iou.sum()), int(floor.sum())
        if q['per_bin'] >= 0:
            got = int(q['bin_first'].sum())
            rest = (q['n_iou_exp'] - got) / (n_iou - got)            # the IoU set's own fill
            p[iou] = rest                                            # outside every interval: the fill only
            for i, first in enumerate(q['bin_first']):
                m = iou & (q['interval'] == i)
                if m.any():
                    p1 = first / m.sum()
                    p[m] = p1 + (1 - p1) * rest
        else:
            p[iou] = q['iou_min'] / max(n_iou, 1)
        p[floor] = q['floor_min'] / max(n_floor, 1)
        if q['n_fill'] > 0:                                          # the final fill from all remaining negatives
            last = q['n_fill'] / (q['n_neg'] - q['iou_min'] - q['floor_min'])
            p[neg] = p[neg] + (1 - p[neg]) * last
    return p


def check_sample(q, assigned, pos_inds, neg_inds):
    """Hold one draw (index arrays into the candidates) to the quotas: the counts the arithmetic fixes are equal,
    those a later uniform fill may raise are lower bounds."""
    a = np.asarray(assigned)
    pos_inds, neg_inds = np.asarray(pos_inds, np.int64), np.asarray(neg_inds, np.int64)
    both = np.concatenate([pos_inds, neg_inds])
    assert len(np.unique(both)) == len(both), 'duplicate index'
    assert both.size == 0 or (both.min() >= 0 and both.max() < len(a))
    assert (a[pos_inds] > 0).all() and (a[neg_inds] == 0).all()
    assert len(pos_inds) == q['k_pos'], (len(pos_inds), q['k_pos'])
    assert len(neg_inds) == q['k_neg'], (len(neg_inds), q['k_neg'])
    if q['pos_case'] in ('fill', 'cut', 'exact'):
        got = np.array([int((a[pos_inds] == g).sum()) for g in q['gt_ids']], np.int64)
        if q['pos_case'] == 'exact':
            assert (got == q['gt_first']).all(), (got, q['gt_first'])
        elif q['pos_case'] == 'fill':       # every gt keeps its first draw, the fill adds to some
            assert (got >= q['gt_first']).all(), (got, q['gt_first'])
        else:                               # a uniform subset of the union of the first draws
            assert (got <= q['gt_first']).all(), (got, q['gt_first'])
    if q['neg_case'] == 'balanced':
        sel = np.zeros(len(a), bool)
        sel[neg_inds] = True
        n_iou, n_floor = int((sel & q['iou_set']).sum()), int((sel & q['floor_set']).sum())
        if q['n_fill'] == 0:
            assert n_iou == q['iou_min'] and n_floor == q['floor_min'], (n_iou, n_floor, q['iou_min'], q['floor_min'])
        else:
            assert n_iou >= q['iou_min'] and n_floor >= q['floor_min']
        if q['per_bin'] >= 0:
            got = np.array([int((sel & q['iou_set'] & (q['interval'] == i)).sum())
                            for i in range(len(q['bin_first']))], np.int64)
            if int(q['bin_first'].sum()) == q['n_iou_exp'] and q['n_fill'] == 0:
                assert (got == q['bin_first']).all(), (got, q['bin_first'])
            else:
                assert (got >= q['bin_first']).all(), (got, q['bin_first'])
