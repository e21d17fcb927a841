"""Launch sequences of the deformable mirror in a rocprofv3 --kernel-trace database of `tools/exp_dm.py --quick`.

    python tools/dm_trace_summary.py <results.db>

Every render / render_stack starts with pm_lattice's scatter kernel and every render_adjoint ends with its gather kernel, so the trace
is cut there: a window from a scatter to the next gather is one render followed by one adjoint (exp_dm.py alternates them), a window
from a scatter to the next scatter with no gather is a render alone.  Prints each distinct window once -- grid size, precision, the
launch sequence, how often it occurred -- and whether any kernel in it is not this library's (PyTorch elementwise / copy kernels).
"""
import re
import sqlite3
import sys
from collections import OrderedDict


def short(name):
    m = re.match(r'(?:void )?pm::(?:\(anonymous namespace\)::)?(\w+)', name)
    if m:
        head = name.split('(long')[0]
        t = 'f64' if 'double' in head else 'f32'
        return f'{m.group(1)}<{t}>'
    return 'NON-LIBRARY:' + name[:60]


def main(path):
    c = sqlite3.connect(path)
    rows = c.execute('select name, grid_x, grid_y, grid_z, workgroup_x, workgroup_y from kernels order by start').fetchall()
    windows, cur = [], None
    for name, gx, gy, gz, wx, wy in rows:
        s = short(name)
        if s.startswith('lattice_scatter'):
            if cur is not None:
                windows.append(cur)
            cur = dict(kind='render', size=(gy, gx, gz), seq=[s])
            continue
        if cur is None:
            continue
        cur['seq'].append(s)
        if s.startswith('lattice_gather'):
            cur['kind'] = 'render+adjoint'
            windows.append(cur)
            cur = None
    if cur is not None:
        windows.append(cur)
    seen = OrderedDict()
    for w in windows:
        key = (w['kind'], w['size'], tuple(w['seq']))
        seen[key] = seen.get(key, 0) + 1
    for (kind, size, seq), n in seen.items():
        foreign = [s for s in seq if s.startswith('NON-LIBRARY')]
        print(f'{kind:15s} grid(threads y,x,z)={size} x{n}  launches={len(seq)}  non-library={len(foreign)}')
        print('    ' + ' -> '.join(seq))


if __name__ == '__main__':
    main(sys.argv[1])
