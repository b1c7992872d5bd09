#!/usr/bin/env python3
"""Device time of BranchingProcesses::PredictOptionPrice (mcg_price_branching: suffix maxima + bounds kernels) on GBM
matrices of a few shapes; dev tool (the judged rows are bench.py's extra.configs).
Environment: BRANCH_SHAPES = "PATHSxSTEPS,..."; BRANCH_BRANCHES = branches per path and date (10); BRANCH_ROUTE / BRANCH_SHIFT =
a route (1 one launch, 2 per date, 3 binned, 4 XCD) and a slice shift forced through mcg_debug_branch_route, for A/B studies
of the routes at one shape."""
import sys,time
sys.path.insert(0,'.')
import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd import _native as N
e=mc.PathEngine(0); e.timing_enable(True)
import os
shapes=[tuple(int(x) for x in s.split("x")) for s in os.environ.get("BRANCH_SHAPES","1000000x50,4000000x50,250000x252").split(",")]
branches=int(os.environ.get("BRANCH_BRANCHES","10"))
route,shift=int(os.environ.get("BRANCH_ROUTE","0")),int(os.environ.get("BRANCH_SHIFT","0"))
if route or shift: e.debug_branch_route(route,shift)
for n,steps in shapes:
    P=e.gbm(20251031,100.0,0.04,0.2,1.0/steps,steps,n)
    ex=list(range(steps))
    e.price_branching(P,0.04,100.0,1.0,1.0/steps,False,branches,ex,7)
    e.timing_reset()
    r=[e.price_branching(P,0.04,100.0,1.0,1.0/steps,False,branches,ex,7) for _ in range(3)]
    ms,c=e.timing_get(N.K_BRANCHING)
    took=' route %d'%e.debug_branch_route() if route or shift else ''
    print(n,steps,'branching kernels ms per call',round(ms/3,3),'launches',c//3,r[0],took)
    P.free()
