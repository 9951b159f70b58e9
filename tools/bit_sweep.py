"""Bit-identity sweep of the plain one-wavefront builds: python tools/bit_sweep.py OUT.npz  (library from CROWDSTEP_LIB), then
python tools/bit_sweep.py --compare A.npz B.npz.  10 / 20 / 25 / 30 / 50 rows x nine SFM / HSFM models at
W = 13 / 7 / 5 / 3 / 4 and the OCC = 4 twins at W = 4200 (25 rows) / 6300 (20) / 4200 (30): 40 substeps, then 107 fused (states, goals) and a
5-substep trace."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["CROWDSTEP_ROW16"] = "0"
import numpy as np
from social_navigation_pyenvs_amd import scenarios as sc
from social_navigation_pyenvs_amd.batched import CrowdWorlds, SFMS

if sys.argv[1] == "--compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    assert sorted(a.files) == sorted(b.files)
    bad = [k for k in a.files if a[k].tobytes() != b[k].tobytes()]
    print("%d arrays compared, %d differ %s" % (len(a.files), len(bad), bad[:5]))
    sys.exit(1 if bad else 0)
shapes = [(10, 13), (20, 7), (25, 5), (30, 3), (50, 4), (25, 4200), (20, 6300), (30, 4200)]
out, variants = {}, set()
for n, W in shapes:
    base = sc.hybrid_worlds(W, n, SFMS[0], seed0=77 + n)
    rw = (np.arange(W) % 2 == 1).astype(np.int32)
    for model in SFMS:
        P = np.tile(sc.default_params(model), (n, 1)).astype(np.float32)
        cw = CrowdWorlds(base[0].astype(np.float32), base[1].astype(np.float32), P, None, None, type=model, all_params_equal=True,
                         respawn_bounds=base[3], respawn_worlds=rw, layout="soa" if W > 1000 else "aos")
        v = cw.step_variant(); variants.add(v.split(" grid")[0])
        assert "LEAN=1" in v and "ROWS_CT=%d" % n in v, v
        cw.step(0.0125, 20); cw.step(0.0125, 20)
        cw.step(0.0125, 107)
        k = "%d_%d_%s" % (n, W, model)
        out[k + "_states"], out[k + "_goals"] = cw.get_states(), cw.get_goals()
        out[k + "_trace"] = cw.step_trace(0.0125, 5)
np.savez(sys.argv[1], **out)
print(len(out), "arrays,", len(variants), "distinct builds")
