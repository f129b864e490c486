"""child process of test_rmq_fwd_queue_refill: MGA_RMQ_WAVES is read once per process.  Three persistent wavefronts take every run of the launch from the queue."""
import sys
import numpy as np
sys.path.insert(0, __file__.rsplit("/", 2)[0])
import minigraph_amd as mga
import rmq_cases as rc

grp = rc.shape_group()
a, runs, where = rc.launch(grp)
assert len(runs) >= 35
f, p, v, status = mga.rmq_fwd_batch(a, runs, **grp.par._asdict())
for c, r0, abs0 in where:
    hf, hp, hv, _ = rc.host_fwd_runs(c.a, c.cuts, grp.par, count_ties=False)
    for r, (beg, end) in enumerate(c.cuts):
        assert status[r0 + r] == c.expect.get(r, 0), (c.name, r, int(status[r0 + r]))
        if status[r0 + r] == 0:
            s = slice(abs0 + beg, abs0 + end)
            assert np.array_equal(f[s], hf[beg:end]) and np.array_equal(p[s], hp[beg:end]) and np.array_equal(v[s], hv[beg:end]), (c.name, r)
print("REFILL-OK", len(runs))
