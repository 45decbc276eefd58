"""Diagnostic (stamps build with STAMPS_EXTRA=-DRRPGO_STAMPS_CHILD): the children of every front on the critical path of the
dataflow factorisation (k_factor_flow), one row per child -- when its flag was set, at which 16-column block of the parent's
panel it was added (0: before the panel), when the parent began to wait for it, how long it waited, and where the parent's
panel stood in time (its start and end).  The critical path is found as scripts/gpu_flow_path.py finds it.
usage: gpu_flow_children.py [intel|input_M3500_g2o|dlr]"""
import ctypes as C, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rustrobotics_amd import _lib
_lib.LIB_PATH = os.path.join(ROOT, 'rustrobotics_amd', 'librr_pgo_stamps.so')
from rustrobotics_amd import PoseGraph
name = sys.argv[1] if len(sys.argv) > 1 else 'intel'
g = PoseGraph.new(os.path.join(ROOT, 'tests/golden/g2o', name + '.g2o'))
g.iterate_async(3); g.sync()
L = _lib.load()
n = C.c_int32()
L.rr_pgo_debug_stamps12(g._h, None, C.byref(n))
S = n.value
out = np.zeros((S, 20))
L.rr_pgo_debug_stamps12(g._h, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n))
st = out[:, :12] * 0.01          # us
block = out[:, 9].astype(int)    # slot 9 is a plain number in this build
parent = out[:, 12].astype(int); nc = out[:, 14].astype(int); nr = out[:, 15].astype(int)
if not bool(out[0, 17]):
    sys.exit('the handle does not run the dataflow launch')
t0 = st[:, 0].min()
kids = {}
for s in range(S):
    if parent[s] >= 0: kids.setdefault(parent[s], []).append(s)
done = st[:, 11]
path, s = [], int(np.argmax(st[:, 6]))
while True:
    path.append(s)
    ks = kids.get(s, [])
    if not ks: break
    s = max(ks, key=lambda c: done[c])
path.reverse()
print(f'{name}: {S} fronts; factorisation span {st[:, 6].max() - t0:.1f} us; times in us from the first front\'s start')
for s in path:
    ks = sorted(kids.get(s, []), key=lambda c: (block[c], done[c]))
    if not ks: continue
    nblk = (nc[s] + 15) // 16
    print(f'front {s}: nc {nc[s]} ({nblk} blocks) nr {nr[s]}; start {st[s, 0] - t0:.1f}, panel {st[s, 3] - t0:.1f} .. {st[s, 4] - t0:.1f}, flag {done[s] - t0:.1f}, waited {st[s, 10]:.1f} in all')
    print('   child   nc   nr | flag at | added at block | wait began | wait ended | waited | flag -> wait ended')
    for c in ks:
        if st[c, 8] == 0:
            print(f'   {c:5d} {nc[c]:4d} {nr[c]:4d} | {done[c] - t0:7.1f} | (same task: no wait)')
            continue
        w0, w1 = st[c, 7] - t0, st[c, 8] - t0
        print(f'   {c:5d} {nc[c]:4d} {nr[c]:4d} | {done[c] - t0:7.1f} | {block[c]:14d} | {w0:10.1f} | {w1:10.1f} | {w1 - w0:6.1f} | {w1 - (done[c] - t0):6.1f}')
