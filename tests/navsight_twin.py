"""The twin of the any-angle paths (vtmc_nav_sight, vtmc_navfield_trace_smooth): a restatement of the NAVSIGHT rule of
include/vtmc_navsight.h in plain Python ints, written from the header's text with no knowledge of the kernels.  The rule is integers only,
so everything test_terrain_navsight.py compares with it must be EQUAL.  Where the device keeps the spans ahead of a waypoint in a ring and
tops it up, the twin collects the chain of every anchor anew and tries its entries from the far end; where the device recovers column
offsets from the links it followed, the twin looks every span's column up in column_offsets.

A walk depends on the nav result (and, for its cost, on the edge costs) alone, so a Walker remembers every walk it has made: the smoothed
traces of many parameter sets over one field share them.

A nav result is (spans, column_offsets, box_lo, box_dims) as Extractor.terrain_nav returns it (nav_twin.build makes the same)."""
import numpy as np

from volumetricterrain_amd._lib import NAVFIELD_UNREACHED, NAVSIGHT_ANY_COST, NAVSIGHT_HIT_DTYPE, NAVSIGHT_MAX_LOOK

ANY = NAVSIGHT_ANY_COST


def columns(nav):
    """(cx, cz) of every span: the column c with column_offsets[c] <= s < column_offsets[c + 1], cx = c % dx, cz = c // dx."""
    spans, offsets, first, ext = nav[:4]
    c = np.searchsorted(np.asarray(offsets), np.arange(len(spans)), side="right") - 1
    dx = max(int(ext[0]), 1)
    return (c % dx).tolist(), (c // dx).tolist()


class Walker:
    def __init__(self, nav, costs=None):
        """costs: navfield_twin.edge_costs of the spans, or None where no walk's cost is asked for (it is then 0)."""
        self.n = len(nav[0])
        self.link = nav[0]["link"].astype(np.int64).tolist()
        self.cost = np.asarray(costs).tolist() if costs is not None else None
        self.cx, self.cz = columns(nav)
        self.seen = {}

    def c(self, s, k):
        return self.cost[s][k] if self.cost is not None else 0

    def follow(self, s, k):
        t = self.link[s][k]
        return t if 0 <= t < self.n else -1   # a link value outside 0..n-1 ends the walk like -1

    def walk(self, a, b):
        """(last, steps, w) of the walk from span a towards span b."""
        key = (a, b)
        if key not in self.seen:
            self.seen[key] = self._walk(a, b)
        return self.seen[key]

    def _walk(self, a, b, trail=None):
        nx, nz = abs(self.cx[b] - self.cx[a]), abs(self.cz[b] - self.cz[a])
        kx = 1 if self.cx[b] > self.cx[a] else 0
        kz = 3 if self.cz[b] > self.cz[a] else 2
        s, i, j, steps, w = a, 0, 0, 0, 0
        while i < nx or j < nz:
            ex, ez = (2 * i + 1) * nz, (2 * j + 1) * nx
            if ex == ez:   # through a corner of four columns: both ways round must exist and meet
                p, q = self.follow(s, kx), self.follow(s, kz)
                if p < 0 or q < 0:
                    break
                t1, t2 = self.follow(p, kz), self.follow(q, kx)
                if t1 < 0 or t2 < 0 or t1 != t2:
                    break
                w += max(self.c(s, kx) + self.c(p, kz), self.c(s, kz) + self.c(q, kx))
                s, i, j, steps = t1, i + 1, j + 1, steps + 2
                if trail is not None:
                    trail += [p, q, t1]
                continue
            k = kx if ex < ez else kz
            t = self.follow(s, k)
            if t < 0:
                break
            w += self.c(s, k)
            s, steps = t, steps + 1
            if trail is not None:
                trail.append(t)
            i, j = (i + 1, j) if ex < ez else (i, j + 1)
        assert steps <= nx + nz
        return s, steps, w

    def visible(self, a, b):
        return self.walk(a, b)[0] == b

    def passed(self, a, b):
        """The spans the walk from a towards b stands on, a first; at a corner both side spans, then the far one."""
        trail = [a]
        assert self._walk(a, b, trail) == self.walk(a, b)
        return trail

    def sight(self, from_spans, to_spans):
        """The hits of the pairs."""
        hits = np.zeros(len(from_spans), NAVSIGHT_HIT_DTYPE)
        for at, (a, b) in enumerate(zip(np.asarray(from_spans).tolist(), np.asarray(to_spans).tolist())):
            assert -1 <= a < self.n and -1 <= b < self.n
            hits[at] = (-1, 0) if a < 0 or b < 0 else self.walk(a, b)[:2]
        return hits

    def smooth(self, cells, starts, max_len, max_look, max_extra_cost=ANY):
        """(paths, lengths) of the smoothed traces of the starts (a span, or -1) over the cells of a field on the same spans."""
        assert 1 <= max_look <= NAVSIGHT_MAX_LOOK and max_len >= 1 and 0 <= max_extra_cost <= ANY
        assert max_extra_cost == ANY or self.cost is not None
        nxt, D = cells["next"].tolist(), cells["cost"].tolist()
        paths, lengths = np.full((len(starts), max_len), -1, np.int32), np.zeros(len(starts), np.int32)
        for at, s0 in enumerate(np.asarray(starts).tolist()):
            assert -1 <= s0 < self.n
            if s0 < 0 or D[s0] == NAVFIELD_UNREACHED:
                continue
            row, a = [s0], s0
            while len(row) < max_len and nxt[a] >= 0:
                chain, s = [], a
                while len(chain) < max_look and nxt[s] >= 0:
                    s = nxt[s]
                    chain.append(s)
                for b in reversed(chain):   # the last entry that passes is the first one found from the far end
                    last, _, w = self.walk(a, b)
                    if last == b and (max_extra_cost == ANY or w + D[b] <= D[a] + max_extra_cost):
                        break
                else:
                    raise AssertionError("span %d: chain[0] is a cheapest step and must pass" % a)
                row.append(b)
                a = b
            paths[at, :len(row)], lengths[at] = row, len(row)
        return paths, lengths
