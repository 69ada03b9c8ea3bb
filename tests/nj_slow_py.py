"""TEST INFRASTRUCTURE: the reference's `-slow` (exhaustiveNJSearch, NJ.tcc:3648-3684) on top of the Python NJ driver.

No top hits (VeryFastTree.cpp:113-115: nDiffAllow = 0, every out-distance recomputed after a join, NJ.tcc:3049-3055) and no
visible set: every join is the pair of active nodes with the lowest criterion, found by `hit.criterion < best.criterion` over
i ascending, j > i ascending - the lexicographically first (i, j) among the pairs that attain the minimum.  The join distance
of two unchanged nodes does not change between joins, so it is computed once (setDistCriterion(lower id, higher id): the
order the reference's loop calls profileDist in) and kept; only the criterion is formed anew at every join, with
setCriterion's arithmetic (NJ.tcc:1099-1107): double arithmetic on the numeric_t distance and the two out-distances, one
rounding to numeric_t.  The product's version is a matrix on the device (veryfasttree_amd/csrc/vft_kernels_exhaustive.h).
"""
import numpy as np

from nj_driver_py import NJDriver


class SlowNJDriver(NJDriver):
    def __init__(self, ops, codes, **kw):
        kw["tophits_mult"] = 0.0   # n_diff_allow = 0
        NJDriver.__init__(self, ops, codes, **kw)
        self.tied_joins = []       # joins whose minimum criterion was attained by more than one pair

    def _distances(self, lo, hi, n_active):
        d, _, _ = self.ops.setDistCriterion(np.asarray(lo, np.int64), np.asarray(hi, np.int64), n_active, 0, self.totdiam)
        return d

    def exhaustive_search(self, n_active):
        act = np.nonzero(self.parent[:self.maxnode] < 0)[0]
        assert len(act) == n_active and (self.n_out[act] == n_active).all()
        out = self.out_dist[act].astype(np.float64)
        crit = (self.dist[np.ix_(act, act)].astype(np.float64) - (out[:, None] + out[None, :]) / float(n_active - 2)).astype(self.dt)
        crit[np.tril_indices(n_active)] = np.inf
        flat = int(np.argmin(crit))   # the first minimum in row-major order = the first (i, j)
        a, b = divmod(flat, n_active)
        if int((crit == crit[a, b]).sum()) > 1:
            self.tied_joins.append(len(self.joins))
        i, j = int(act[a]), int(act[b])
        return i, j, self.dist[i, j], crit[a, b]

    def after_join(self, i, j, newnode, n_active):
        """hook: the join is complete (n_active = the count after it, every out-distance current)"""

    def run(self, max_joins=None):
        n, dt, ops = self.n_seqs, self.dt, self.ops
        self.dist = np.full((self.maxnodes, self.maxnodes), np.inf, dt)   # [lower id, higher id]
        iu = np.triu_indices(n, 1)
        self.dist[iu] = self._distances(iu[0], iu[1], n)
        n_active_reset = n_active = n
        while n_active > 3:
            if max_joins is not None and len(self.joins) >= max_joins:
                break
            i, j, dist_ij, crit = self.exhaustive_search(n_active)
            newnode = self.maxnode
            self.maxnode += 1
            self.parent[i] = self.parent[j] = newnode
            self.child[newnode] = (i, j)
            self.joins.append((i, j, newnode, float(crit)))
            delta = float(dt(self.out_dist[i] - self.out_dist[j])) / float(n_active - 2)
            self.branchlength[i] = dt((float(dist_ij) + delta) / 2)
            self.branchlength[j] = dt((float(dist_ij) - delta) / 2)
            self.diameter[newnode] = dt(0.5 * float(dt(self.branchlength[i] + self.diameter[i])) +
                                        0.5 * float(dt(self.branchlength[j] + self.diameter[j])))
            ops.set_max_node(self.maxnode)
            ops.averageProfile([newnode], [i], [j])
            ops.set_parents(i, [newnode])
            ops.set_parents(j, [newnode])
            ops.set_node_scalars(newnode, diameter=np.array([self.diameter[newnode]], dt))
            changed = n_active_reset - (n_active - 1)
            if changed >= self.n_reset_out_profile and changed >= self.f_reset_out_profile * n_active_reset:
                active = np.nonzero(self.parent[:self.maxnode] < 0)[0]
                tot = 0.0
                for v in active:
                    tot += float(self.diameter[v])
                self.totdiam = tot
                ops.outProfile(active)
                n_active_reset = n_active - 1
            else:
                ops.updateOutProfile(i, j, newnode, n_active)
                self.totdiam += float(dt(dt(self.diameter[newnode] - self.diameter[i]) - self.diameter[j]))
            ops.set_out_distances(newnode, np.zeros(1, dt), np.array([10 * n]))
            n_active -= 1
            ops.setOutDistance(None, n_active, self.totdiam)   # NJ.tcc:3049-3055
            self._sync_out()
            others = np.nonzero(self.parent[:newnode] < 0)[0]
            self.dist[others, newnode] = self._distances(others, np.full(len(others), newnode), n_active)
            self.after_join(i, j, newnode, n_active)
        return self.joins
