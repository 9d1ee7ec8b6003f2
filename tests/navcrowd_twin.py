"""The twin of the crowd (vtmc_navcrowd_spawn, _step, _read, _info): a restatement of the NAVCROWD rule of include/vtmc_navcrowd.h in plain
Python ints, written from the header's text with no knowledge of the kernels.  Where the device runs a tick as two launches and lets an
atomicMin on a claim word decide, the twin walks the agents one after the other over a copy of the occupancy as the tick found it, keeps
the claims in a dict and settles them afterwards; the candidates are a sorted list.  The rule is integers only, so everything
test_terrain_navcrowd.py compares with it must be EQUAL, as bytes.

It also counts, over all ticks since the spawn: `moves`; `lost`, the claims that went to a smaller index; `sidesteps`, the claims of a
candidate that was not the first; and keeps `trail`, every move as (tick, agent, from, to), for the tests of the rule's properties.

links are a nav result's spans["link"]; cells a NAVFIELD_CELL_DTYPE array; costs navfield_twin.edge_costs of the spans."""
import numpy as np

from volumetricterrain_amd._lib import (NAVCROWD_AGENT_DTYPE, NAVCROWD_ANY_DETOUR, NAVCROWD_ARRIVED, NAVCROWD_BUDGET_CAP, NAVCROWD_GONE, NAVCROWD_LEAVE_ON_ARRIVAL,
                                        NAVCROWD_MAX_SPEED, NAVCROWD_STRANDED, NAVCROWD_UNPLACED, NAVCROWD_WALKING, NAVFIELD_UNREACHED)

ANY = NAVCROWD_ANY_DETOUR
WALKING, ARRIVED, STRANDED, GONE, UNPLACED = NAVCROWD_WALKING, NAVCROWD_ARRIVED, NAVCROWD_STRANDED, NAVCROWD_GONE, NAVCROWD_UNPLACED
OCCUPYING = (WALKING, ARRIVED, STRANDED)


class Crowd:
    def __init__(self, links, cells=None, costs=None):
        self.link = np.asarray(links).astype(np.int64).tolist()
        self.n = len(self.link)
        self.agents = []          # [span, budget, speed, state] per agent
        self.occupancy = [-1] * self.n
        self.ticks = self.moved_last = 0
        self.moves = self.lost = self.sidesteps = 0
        self.trail = []
        if cells is not None:
            self.set_field(cells, costs)

    def set_field(self, cells, costs):
        """A new field on the same spans: the crowd stays (the re-route)."""
        assert len(cells) == self.n and len(costs) == self.n
        self.D, self.next, self.cost = cells["cost"].astype(np.int64).tolist(), cells["next"].astype(np.int64).tolist(), np.asarray(costs).astype(np.int64).tolist()

    def spawn(self, spans, speeds):
        """Spawn: replaces the crowd; returns the number of placed agents."""
        spans = [int(s) for s in spans]
        speeds = [int(speeds)] * len(spans) if np.ndim(speeds) == 0 else [int(v) for v in speeds]
        assert len(spans) == len(speeds) >= 1 and all(-1 <= s < self.n for s in spans) and all(1 <= v <= NAVCROWD_MAX_SPEED for v in speeds)
        self.occupancy = [-1] * self.n
        self.agents = []
        for i, (s, v) in enumerate(zip(spans, speeds)):
            if s >= 0 and self.occupancy[s] < 0:   # in index order: the smallest index of those that ask for s
                self.occupancy[s] = i
                self.agents.append([s, 0, v, WALKING])
            else:
                self.agents.append([-1, 0, v, UNPLACED])
        self.ticks = self.moved_last = self.moves = self.lost = self.sidesteps = 0
        self.trail = []
        return sum(a[3] == WALKING for a in self.agents)

    def candidates(self, s, max_detour):
        """Tick, steps 5 and 6: (D(t) + c, k, t, c) of the candidates of span s, in their order."""
        out = []
        for k in range(4):
            t = self.link[s][k]
            if not 0 <= t < self.n or self.D[t] == NAVFIELD_UNREACHED or not self.D[t] < self.D[s]:
                continue
            c = self.cost[s][k]
            if max_detour != ANY and self.D[t] + c > self.D[s] + max_detour:
                continue
            out.append((self.D[t] + c, k, t, c))
        return sorted(out)

    def tick(self, max_detour, flags):
        before = list(self.occupancy)     # what every decision of this tick reads
        claims, leaving = {}, []
        for i, a in enumerate(self.agents):
            s = a[0]
            if a[3] in (GONE, UNPLACED):
                continue
            if self.D[s] == NAVFIELD_UNREACHED:
                a[3] = STRANDED
                continue
            if self.next[s] == -1:
                a[3] = GONE if flags & NAVCROWD_LEAVE_ON_ARRIVAL else ARRIVED
                if a[3] == GONE:
                    leaving.append(s)
                continue
            a[3] = WALKING
            a[1] = min(a[1] + a[2], NAVCROWD_BUDGET_CAP)
            order = self.candidates(s, max_detour)
            assert order and order[0][2] == self.next[s] and order[0][0] == self.D[s], "the first candidate is next(s)"
            free = [x for x in order if before[x[2]] < 0]
            if not free or a[1] < free[0][3]:
                continue
            _, k, t, c = free[0]
            self.sidesteps += free[0] != order[0]
            claims.setdefault(t, []).append((i, c))
        moved = 0
        for t, who in claims.items():
            i, c = min(who)
            self.lost += len(who) - 1
            a = self.agents[i]
            self.trail.append((self.ticks, i, a[0], t))
            self.occupancy[a[0]], self.occupancy[t] = -1, i
            a[0], a[1] = t, a[1] - c
            moved += 1
        for s in leaving:                 # free from the next tick on
            self.occupancy[s] = -1
        self.ticks, self.moved_last, self.moves = self.ticks + 1, moved, self.moves + moved

    def step(self, max_detour=ANY, flags=0, n_ticks=1):
        assert self.agents and flags in (0, NAVCROWD_LEAVE_ON_ARRIVAL)
        for _ in range(n_ticks):
            self.tick(max_detour, flags)
        return self.info()

    def read(self):
        """(agents, occupancy) as Extractor.navcrowd_read returns them."""
        agents = np.zeros(len(self.agents), NAVCROWD_AGENT_DTYPE)
        for i, (s, b, v, st) in enumerate(self.agents):
            agents[i] = (s, b, v, st)
        return agents, np.asarray(self.occupancy, np.int32)

    def info(self):
        """Info: (agents, occupying, arrived, ticks, moves of the last tick)."""
        states = [a[3] for a in self.agents]
        return (len(states), sum(st in OCCUPYING for st in states), sum(st in (ARRIVED, GONE) for st in states), self.ticks, self.moved_last)
