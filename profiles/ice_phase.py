"""Cost of frazil ice formation (pop_init_ice): the HIP-event time of the "ice" phase (k_ice_formation on the new
tracers) beside the "correct" phase of the same context, PopModel.time_phase, at the gx1v7 and tx0.1v3 shapes with CESM's ice_nml
(kmxice = 1, virtual salt flux, 'mushy'), and the STEP timer over five steps that form ice.

    python profiles/ice_phase.py            # one line of JSON per shape
"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge
from popcfg import named_config
pkg = ge.load_package()
out = {}
for name in ("gx1v7", "tx0.1v3"):
    m = pkg.PopModel(named_config(name))
    m.init_ice(ice_freq_opt="coupled", licecesm2=1, kmxice=1, lactive_ice=1, lfw_as_salt_flx=1, tfreeze_option="mushy")
    for _ in range(4):
        m.step()
    m.sync()
    r = {}
    for rep in range(3):
        for ph in ("ice", "correct"):
            r.setdefault(ph, []).append(m.time_phase(ph, 20))
    m.timers_reset()
    for _ in range(5):
        m.step()
    m.sync()
    r["step_ms"] = m.timer("STEP")[0] / 5
    out[name] = r
    print(name, json.dumps(r), flush=True)
    m.close()
