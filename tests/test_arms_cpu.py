"""The ledger of kernel arms (CPU, no GPU): every ``getenv("BGS_...")`` of the HIP sources, every ``BGS_*`` environment
read of the package's Python files and every prototype of include/bgs_tuning.h has a row in ``tests.arm_problems.ARMS`` that
names the test which holds the arm to its relation with the default, or carries a written exemption.  An arm added later
without a test fails here."""
import glob
import os
import re

from tests.arm_problems import ARMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'balancedgroupsoftmax_amd')
EXEMPTIONS = ('ablate', 'policy', 'debug', 'query')


def _read(path):
    with open(path, errors='replace') as f:
        return f.read()


def _csrc_getenv():
    """name -> [files] of every ``getenv("BGS_...")`` under csrc/ (kernel and header files)."""
    found = {}
    for path in sorted(glob.glob(os.path.join(PKG, 'csrc', '*'))):
        if not os.path.isfile(path) or not path.endswith(('.hip', '.h', '.hpp', '.cpp')):
            continue
        for name in re.findall(r'getenv\(\s*"(BGS_[A-Z0-9_]+)"', _read(path)):
            found.setdefault(name, []).append(os.path.basename(path))
    return found


def _python_env_reads():
    found = {}
    for path in sorted(glob.glob(os.path.join(PKG, '*.py'))):
        for name in re.findall(r'''(?:environ(?:\.get|\.setdefault|\.pop)?\s*[\(\[]|getenv\()\s*['"](BGS_[A-Z0-9_]+)['"]''', _read(path)):
            found.setdefault(name, []).append(os.path.basename(path))
    return found


def _header_prototypes():
    text = re.sub(r'/\*.*?\*/', '', _read(os.path.join(ROOT, 'include', 'bgs_tuning.h')), flags=re.S)
    return sorted(set(re.findall(r'^\s*(?:void|int|size_t)\s+(bgs_[a-z0-9_]+)\s*\(', text, flags=re.M)))


def _ablate_only(name):
    """Every ``getenv("name")`` of csrc/ sits between ``#ifdef BGS_ABLATE`` and its ``#endif`` / ``#else``."""
    hits = 0
    for path in glob.glob(os.path.join(PKG, 'csrc', '*.hip')):
        depth = []                                      # stack of (is the BGS_ABLATE block)
        for line in _read(path).split('\n'):
            s = line.strip()
            if s.startswith('#if'):
                depth.append(bool(re.match(r'#\s*ifdef\s+BGS_ABLATE\b', s)))
            elif s.startswith('#else') and depth:
                depth[-1] = False
            elif s.startswith('#endif') and depth:
                depth.pop()
            if 'getenv("%s")' % name in line:
                hits += 1
                if not any(depth):
                    return False
    return hits > 0


def test_the_scans_find_the_known_switches():
    """The three scans see what they are meant to see (a regular expression that matches nothing would pass the ledger)."""
    c, p, h = _csrc_getenv(), _python_env_reads(), _header_prototypes()
    assert len(c) >= 40 and {'BGS_NMS_SCAN', 'BGS_HALO_FB32', 'BGS_WGRAD_NBUF', 'BGS_BFX_PLANES3_NB'} <= set(c)
    assert len(p) >= 15 and {'BGS_CONV_MATH', 'BGS_FUSED_SGD', 'BGS_LIB_PATH', 'BGS_PROPOSAL_TAIL'} <= set(p)
    assert len(h) >= 30 and {'bgs_conv_bf16s_tuning', 'bgs_gs_head_tuning', 'bgs_launch_census'} <= set(h)
    assert not any(n.startswith('BGS_CENSUS') or n in ('BGS_OK', 'BGS_MAX_BINS') for n in p)


def test_every_switch_and_hook_has_a_row():
    found = dict(_csrc_getenv())
    found.update(_python_env_reads())
    found.update({n: ['bgs_tuning.h'] for n in _header_prototypes()})
    missing = sorted(n for n in found if n not in ARMS)
    assert not missing, 'arms without a test or an exemption in tests/arm_problems.py ARMS: %s' % \
        ', '.join('%s (%s)' % (n, ', '.join(found[n])) for n in missing)
    stale = sorted(n for n in ARMS if n not in found)
    assert not stale, 'rows of ARMS whose switch or hook is gone: %s' % ', '.join(stale)


def test_every_row_names_an_existing_test_or_an_allowed_exemption():
    sources = {}
    bad = []
    for name, row in sorted(ARMS.items()):
        kind = row.get('exempt')
        if kind is None:
            if not row.get('test') or not row.get('relation'):
                bad.append((name, 'neither a test with its relation nor an exemption'))
        elif kind not in EXEMPTIONS or not row.get('why'):
            bad.append((name, 'exemption %r without a reason or not one of %s' % (kind, EXEMPTIONS)))
        elif kind == 'policy' and not row.get('test'):
            bad.append((name, 'a policy switch names the test that already covers it'))
        elif kind == 'ablate' and not _ablate_only(name):
            bad.append((name, 'read outside #ifdef BGS_ABLATE'))
        elif kind == 'debug' and 'debug' not in name:
            bad.append((name, 'not a debug hook'))
        elif kind == 'query' and not name.startswith('bgs_'):
            bad.append((name, 'only header entries report'))
        for test_id in (row.get('test') or '').split(' / '):
            if not test_id:
                continue
            m = re.match(r'^(tests\.[a-z0-9_]+)::(test_[A-Za-z0-9_]+)(\[.*\])?$', test_id)
            if not m:
                bad.append((name, 'malformed test id %r' % test_id))
                continue
            path = os.path.join(ROOT, *m.group(1).split('.')) + '.py'
            if path not in sources:
                sources[path] = _read(path) if os.path.exists(path) else ''
            if not re.search(r'^def %s\(' % re.escape(m.group(2)), sources[path], flags=re.M):
                bad.append((name, 'no such test: %s' % test_id))
            elif m.group(3) and m.group(3)[1:-1].split('-')[0] not in sources[path]:
                bad.append((name, 'no such case: %s' % test_id))
    assert not bad, bad
