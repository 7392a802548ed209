"""TEST INFRASTRUCTURE ONLY — never imported by the product (erasure-codes-prototype_amd/).

Pure-Python restatement of the reference's partitioning and repair planning: the
PlacementRule partitions (erasure_code.cpp:150-169, rs.cpp:78-116, lrc.cpp:215-238 / per-class
partition_optimal, pc.cpp:378-443 / 1091-1158), check_if_decodable for every LRC variant, and
generate_repair_plan with its help-block selection (rs.cpp:118-279, lrc.cpp:240-574 / 1757-2023,
pc.cpp:451-551 / 1166-1264).  Used by tests/test_planning.py to pin csrc/planning.cpp.

Parity status: the reference's planning is self-contained C++ (no Jerasure), so this restatement is
checked line by line against its source, and pinned by the plans the reference's own classes returned
(tests/golden/reference_ec.json, tests/test_reference_ec.py) besides the hand-derived expectations in
tests/test_planning.py (the SURVEY.md §8(d) config-3 partition, RS/PC examples worked by hand).
Two conventions shared with the product and documented there:
  * "largest first" orderings are libstdc++'s std::sort, ties included (_std_sort below; stable up to 16 elements);
  * random placement uses the splitmix64 stream below instead of random_device-seeded mt19937.
"""
from __future__ import annotations

from dataclasses import dataclass, field

FLAT, RANDOM, OPTIMAL, SUB_OPTIMAL = 0, 1, 2, 3
_M64 = (1 << 64) - 1


@dataclass
class RepairPlan:  # erasure_code.h:53-58
    local_or_column: bool = False
    failure_idxs: list = field(default_factory=list)
    help_blocks: list = field(default_factory=list)


def _std_sort(v, comp):
    """std::sort as libstdc++ implements it (bits/stl_algo.h: __introsort_loop with its 16-element threshold and
    median-of-three pivot moved to the front, then __final_insertion_sort), in place.  The reference sorts its
    (partition, size) pairs with it under a comparator that ties on equal sizes (utils.cpp:159-162), so above 16
    elements the order of the ties -- and with it which helpers a plan names first -- is this algorithm's, and the
    reference's own classes (tests/golden/reference_ec.json) show exactly that order.  Up to 16 elements it is a
    stable insertion sort.  The heapsort the loop falls back to after 2 * floor(log2 n) bad splits is not restated."""
    n = len(v)

    def linear_insert(last):  # __unguarded_linear_insert
        val = v[last]
        nxt = last - 1
        while comp(val, v[nxt]):
            v[last] = v[nxt]
            last = nxt
            nxt -= 1
        v[last] = val

    def insertion(first, last):  # __insertion_sort
        for i in range(first + 1, last):
            if comp(v[i], v[first]):
                val = v[i]
                v[first + 1:i + 1] = v[first:i]
                v[first] = val
            else:
                linear_insert(i)

    def median_to_first(result, a, b, c):  # __move_median_to_first
        if comp(v[a], v[b]):
            pick = b if comp(v[b], v[c]) else (c if comp(v[a], v[c]) else a)
        else:
            pick = a if comp(v[a], v[c]) else (c if comp(v[b], v[c]) else b)
        v[result], v[pick] = v[pick], v[result]

    def partition(first, last, pivot):  # __unguarded_partition
        while True:
            while comp(v[first], v[pivot]):
                first += 1
            last -= 1
            while comp(v[pivot], v[last]):
                last -= 1
            if not first < last:
                return first
            v[first], v[last] = v[last], v[first]
            first += 1

    def loop(first, last, depth):  # __introsort_loop
        while last - first > 16:
            if depth == 0:
                raise NotImplementedError("std::sort's heapsort fallback")
            depth -= 1
            median_to_first(first, first + 1, first + (last - first) // 2, last - 1)
            cut = partition(first + 1, last, first)
            loop(cut, last, depth)
            last = cut

    if n:
        loop(0, n, 2 * (n.bit_length() - 1))
        if n > 16:  # __final_insertion_sort
            insertion(0, 16)
            for i in range(16, n):
                linear_insert(i)
        else:
            insertion(0, n)
    return v


def _desc(pairs):
    """std::sort(..., cmp_descending) (utils.cpp:159-162): descending on .second, ties as libstdc++ leaves them."""
    return _std_sort(list(pairs), lambda a, b: a[1] > b[1])


class Planner:
    def __init__(self, k, m):
        self.k, self.m = k, m
        self.placement_rule = OPTIMAL
        self.partition_plan = []
        self.local_or_column = False
        self._rng = None

    # ---- random_range / random_index (utils.cpp:6-21) over a splitmix64 stream
    def set_random_seed(self, seed):
        self._rng = seed & _M64

    def _next(self):
        self._rng = (self._rng + 0x9E3779B97F4A7C15) & _M64
        z = self._rng
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)

    def random_range(self, lo, hi):
        return lo + self._next() % (hi - lo + 1)

    def random_index(self, n):
        return self._next() % n

    def partition_flat(self):  # erasure_code.cpp:150-157
        self.partition_plan += [[i] for i in range(self.k + self.m)]

    def generate_partition(self):  # erasure_code.cpp:159-169
        self.partition_plan = []
        if self.placement_rule == FLAT:
            self.partition_flat()
        elif self.placement_rule == RANDOM:
            self.partition_random()
        elif self.placement_rule == OPTIMAL:
            self.partition_optimal()
        elif self.placement_rule == SUB_OPTIMAL:
            self.partition_sub_optimal()
        return self.partition_plan

    def _random_blocks(self, n, max_size):  # rs.cpp:78-101 / lrc.cpp:215-238
        blocks = list(range(n))
        cnt = 0
        while cnt < n:
            size = min(self.random_range(1, max_size), n - cnt)
            part = []
            for _ in range(size):
                part.append(blocks.pop(self.random_index(n - cnt)))
                cnt += 1
            self.partition_plan.append(part)


class RS(Planner):
    def partition_random(self):
        self._random_blocks(self.k + self.m, self.m)

    def partition_optimal(self):  # rs.cpp:103-116
        n = self.k + self.m
        for s in range(0, n, self.m):
            self.partition_plan.append(list(range(s, min(n, s + self.m))))

    def check_if_decodable(self, f):  # rs.cpp:68-76
        return self.m >= len(f)

    def help_single(self, fi):  # rs.cpp:118-180
        pp, k = self.partition_plan, self.k
        if not pp:
            return []
        main = next(i for i, p in enumerate(pp) if fi in p)
        others = _desc([(i, len(p)) for i, p in enumerate(pp) if fi not in p])
        out, cnt = [], 0
        mh = []
        for b in pp[main]:
            if b != fi:
                if cnt < k:
                    mh.append(b)
                    cnt += 1
                else:
                    break
        if cnt > 0:
            out.append(mh)
        if cnt == k:
            return out
        for i, _ in others:
            h = []
            for b in pp[i]:
                if cnt < k:
                    h.append(b)
                    cnt += 1
                else:
                    break
            if 0 < cnt <= k:
                out.append(h)
            if cnt == k:
                return out
        return out

    def help_multi(self, fs):  # rs.cpp:182-262
        pp, k = self.partition_plan, self.k
        if not pp:
            return []
        part = [list(p) for p in pp]
        fc = [0] * len(pp)
        for f in fs:
            for i, p in enumerate(part):
                if f in p:
                    fc[i] += 1
                    p.remove(f)
                    break
        mains = _desc([(i, len(part[i])) for i in range(len(pp)) if fc[i]])
        others = _desc([(i, len(part[i])) for i in range(len(pp)) if not fc[i]])
        out, cnt = [], 0
        for i, _ in mains + others:
            h = []
            for b in part[i]:
                if cnt < k:
                    h.append(b)
                    cnt += 1
                else:
                    break
            if 0 < cnt <= k and h:
                out.append(h)
            if cnt == k:
                return out
        return out

    def generate_repair_plan(self, fs):  # rs.cpp:264-279
        p = RepairPlan(False, list(fs), self.help_single(fs[0]) if len(fs) == 1 else self.help_multi(fs))
        return True, [p]


class LRC(Planner):
    def __init__(self, k, l, g):  # lrc.h:17-23
        super().__init__(k, l + g)
        self.l, self.g = l, g
        self.r = (k + l - 1) // l

    def partition_random(self):  # lrc.cpp:215-238
        self._random_blocks(self.k + self.l + self.g, self.g + 1)

    def partition_optimal(self):  # lrc.h:75 (no-op in the base class)
        pass

    def partition_sub_optimal(self):
        raise ValueError("sub-optimal placement is Azure-only")

    def check_if_decodable(self, f):  # lrc.h:59
        return True

    def _grouped_optimal(self):  # lrc.cpp:1071-1088, 1284-1301, 2287-2304
        for grp in self.grouping_information()[:self.l]:
            for j in range(0, len(grp), self.g + 1):
                self.partition_plan.append(grp[j:j + self.g + 1])

    def _azure_optimal(self):  # lrc.cpp:725-814 (== 1660-1749)
        k, l, g, r = self.k, self.l, self.g, self.r
        groups = self.grouping_information()
        rem = []
        for grp in groups[:l]:
            for j in range(0, len(grp), g + 1):
                if j + g + 1 > len(grp):
                    rem.append(grp[j:])
                    break
                self.partition_plan.append(grp[j:j + g + 1])
        theta = l
        if (r + 1) % (g + 1) > 1:
            theta = g // ((r + 1) % (g + 1) - 1)
        for i in range(0, len(rem), theta):
            self.partition_plan.append([b for grp in rem[i:i + theta] for b in grp])
        space = []
        for i, p in enumerate(self.partition_plan):
            ng = sum(1 for b in p if b >= k + g) or 1
            space.append((i, g + ng - len(p)))
        left_g, gi = g, k
        if sum(s for _, s in space) >= g:
            for j, s in _desc(space):
                if left_g <= 0:
                    break
                if s > 0:
                    take = s if left_g >= s else left_g
                    left_g -= take
                    for _ in range(take):
                        self.partition_plan[j].append(gi)
                        gi += 1
        else:
            self.partition_plan.append(list(range(gi, k + g)))

    def help_single(self, fi):  # lrc.cpp:240-323
        pp, k, g = self.partition_plan, self.k, self.g
        if not pp:
            return []
        out = []
        if self.local_or_column:
            gid = self.bid2gid(fi)
            for p in pp:
                h = [b for b in p if self.bid2gid(b) == gid and b != fi]
                if h:
                    out.append(h)
            return out
        main, lst = 0, []
        for i, p in enumerate(pp):
            cnt = 0
            for b in p:
                if b < k + g and b != fi:
                    cnt += 1
                if b == fi:
                    main, cnt = i, 0
                    break
            if cnt > 0:
                lst.append((i, cnt))
        cnt, mh = 0, []
        for b in pp[main]:
            if b != fi and b < k + g:
                if cnt < k:
                    mh.append(b)
                    cnt += 1
                else:
                    break
        if cnt > 0:
            out.append(mh)
        if cnt == k:
            return out
        for i, _ in _desc(lst):
            h = []
            for b in pp[i]:
                if b < k + g:
                    if cnt < k:
                        h.append(b)
                        cnt += 1
                    else:
                        break
            if 0 < cnt <= k:
                out.append(h)
            if cnt == k:
                return out
        return out

    def help_multi(self, fs):  # lrc.cpp:325-443
        k, l, g = self.k, self.l, self.g
        flag = len(fs) > g or any(f >= k + g for f in fs)
        pp = self.partition_plan
        if not pp:
            return []
        part = [list(p) for p in pp]
        if flag:
            for f in fs:
                for p in part:
                    if f in p:
                        p.remove(f)
                        break
            return [p for p in part if p]
        fc = [0] * len(pp)
        for f in fs:
            for i, p in enumerate(part):
                if f in p:
                    fc[i] += 1
                    p.remove(f)
                    break
        for lp in range(k + g, k + g + l):
            for p in part:
                if lp in p:
                    p.remove(lp)
                    break
        mains = _desc([(i, len(part[i])) for i in range(len(pp)) if fc[i]])
        others = _desc([(i, len(part[i])) for i in range(len(pp)) if not fc[i]])
        out, cnt = [], 0
        for i, _ in mains + others:
            h = []
            for b in part[i]:
                if cnt < k:
                    h.append(b)
                    cnt += 1
                else:
                    break
            if 0 < cnt <= k and h:
                out.append(h)
            if cnt == k:
                return out
        return out

    def generate_repair_plan(self, fs):  # lrc.cpp:445-574
        k, l, g = self.k, self.l, self.g
        n = k + g + l
        if not self.check_if_decodable(fs):
            return False, []
        plans = []
        if len(fs) == 1:
            loc = self.bid2gid(fs[0]) < l
            self.local_or_column = loc
            plans.append(RepairPlan(loc, list(fs), self.help_single(fs[0])))
            return True, plans
        failed = [0] * n
        gc = [0] * (l + 1)
        ndg, nf = 0, len(fs)
        for f in fs:
            failed[f] = 1
            gc[self.bid2gid(f)] += 1
            if f < k + g:
                ndg += 1
        it = 0
        while nf > 0:
            for gid in range(l):
                if gc[gid] == 1:
                    fi = next(i for i in range(n) if failed[i] and self.bid2gid(i) == gid)
                    self.local_or_column = True
                    plans.append(RepairPlan(True, [fi], self.help_single(fi)))
                    failed[fi] = 0
                    gc[gid] = 0
                    nf -= 1
                    if fi < k + g:
                        ndg -= 1
            if 0 < ndg <= g:
                p = RepairPlan(False, [i for i in range(k + g) if failed[i]], [])
                if len(p.failure_idxs) == 1:
                    self.local_or_column = False
                    p.help_blocks = self.help_single(p.failure_idxs[0])
                else:
                    p.help_blocks = self.help_multi(p.failure_idxs)
                plans.append(p)
                for i in range(k + g):
                    if failed[i]:
                        failed[i] = 0
                        nf -= 1
                        gc[self.bid2gid(i)] -= 1
                ndg = 0
            if it > 0 and nf > 0:
                if not self.check_if_decodable(fs):
                    return False, plans
                p = RepairPlan(False, [i for i in range(n) if failed[i]], [])
                p.help_blocks = self.help_multi(p.failure_idxs)
                plans.append(p)
                for i in range(n):
                    if failed[i]:
                        failed[i] = 0
                        nf -= 1
                        gc[self.bid2gid(i)] -= 1
                ndg = 0
            it += 1
        return True, plans


class AzureLRC(LRC):
    def bid2gid(self, b):  # lrc.cpp:665-676
        k, g = self.k, self.g
        return b // self.r if b < k else (self.l if b < k + g else b - k - g)

    def grouping_information(self):  # lrc.cpp:706-723
        k, l, g, r = self.k, self.l, self.g, self.r
        groups, idx = [], 0
        for i in range(l):
            gs = min(r, k - i * r)
            groups.append(list(range(idx, idx + max(gs, 0))) + [k + g + i])
            idx += max(gs, 0)
        groups.append(list(range(idx, idx + g)))
        return groups

    def partition_optimal(self):
        self._azure_optimal()

    def partition_sub_optimal(self):  # lrc.cpp:816-873
        k, l, g, r = self.k, self.l, self.g, self.r
        rem = []
        for grp in self.grouping_information()[:l]:
            for j in range(0, len(grp), g + 1):
                if j + g + 1 > len(grp):
                    rem.append(grp[j:])
                    break
                self.partition_plan.append(grp[j:j + g + 1])
        theta = l
        if (r + 1) % (g + 1) > 1:
            theta = g // ((r + 1) % (g + 1) - 1)
        for i in range(0, len(rem), theta):
            self.partition_plan.append([b for grp in rem[i:i + theta] for b in grp])
        if theta == len(rem):
            self.partition_plan[-1] += list(range(k, k + g))
        else:
            self.partition_plan.append(list(range(k, k + g)))

    def check_if_decodable(self, fs):  # lrc.cpp:576-620
        k, l, g, r = self.k, self.l, self.g, self.r
        fd, slp, sgp = [0] * l, [1] * l, g
        for b in fs:
            if b < k:
                fd[b // r] += 1
            elif b < k + g:
                sgp -= 1
            else:
                slp[b - k - g] -= 1
        for i in range(l):
            if slp[i] and slp[i] <= fd[i]:
                fd[i] -= slp[i]
                slp[i] = 0
        for i in range(l):
            if sgp >= fd[i]:
                sgp -= fd[i]
            else:
                return False
        return True


class AzureLRC1(LRC):
    def __init__(self, k, l, g):  # lrc.h:113-118
        super().__init__(k, l, g)
        self.r = (k + l - 2) // (l - 1)

    def bid2gid(self, b):  # lrc.cpp:1008-1019
        k, g = self.k, self.g
        return b // self.r if b < k else (self.l - 1 if b < k + g else b - k - g)

    def grouping_information(self):  # lrc.cpp:1051-1069
        k, l, g, r = self.k, self.l, self.g, self.r
        groups, idx = [], 0
        for i in range(l - 1):
            gs = max(min(r, k - i * r), 0)
            groups.append(list(range(idx, idx + gs)) + [k + g + i])
            idx += gs
        groups.append(list(range(idx, idx + g)) + [k + g + l - 1])
        return groups

    def partition_optimal(self):
        self._grouped_optimal()

    def check_if_decodable(self, fs):  # lrc.cpp:881-931
        k, l, g, r = self.k, self.l, self.g, self.r
        fd, slp, sgp = [0] * l, [1] * l, g
        for b in fs:
            if b < k:
                fd[b // r] += 1
            elif b < k + g:
                sgp -= 1
            else:
                slp[b - k - g] -= 1
        for i in range(l):
            if i < l - 1:
                if slp[i] and slp[i] <= fd[i]:
                    fd[i] -= slp[i]
                    slp[i] = 0
            elif slp[i] and sgp == g - 1:
                sgp += 1
        for i in range(l):
            if sgp >= fd[i]:
                sgp -= fd[i]
            else:
                return False
        return True


class _MixedLRC(LRC):  # Opt_LRC / Uni_Cau_LRC: groups over data + global parities
    def __init__(self, k, l, g):  # lrc.h:141-146 / 212-217
        super().__init__(k, l, g)
        self.r = (k + g + l - 1) // l

    def bid2gid(self, b):  # lrc.cpp:1236-1245 / 2241-2250
        return b // self.r if b < self.k + self.g else b - self.k - self.g

    def grouping_information(self):  # lrc.cpp:1270-1282 / 2273-2285
        k, l, g, r = self.k, self.l, self.g, self.r
        groups, idx = [], 0
        for i in range(l):
            gs = max(min(r, k + g - i * r), 0)
            groups.append(list(range(idx, idx + gs)) + [k + g + i])
            idx += gs
        return groups

    def partition_optimal(self):
        self._grouped_optimal()

    def check_if_decodable(self, fs):  # lrc.cpp:1096-1166 == 2025-2095
        k, l, g, r = self.k, self.l, self.g, self.r
        fd, fgp, slp, pure, sgp = [0] * l, [0] * l, [1] * l, [], g
        idx = 0
        for i in range(l):
            gs = min(r, k + g - i * r)
            idx += max(gs, 0)
            pure.append(idx <= k or idx - gs >= k)
        for b in fs:
            if b < k:
                fd[b // r] += 1
            elif b < k + g:
                fgp[b // r] += 1
                sgp -= 1
            else:
                slp[b - k - g] -= 1
        for i in range(l):
            if slp[i] and pure[i]:
                if slp[i] <= fd[i]:
                    fd[i] -= slp[i]
                    slp[i] = 0
                if slp[i] and slp[i] == fgp[i]:
                    fgp[i] -= slp[i]
                    slp[i] = 0
                    sgp += 1
            elif slp[i] and not pure[i]:
                if fd[i] == 1 and not fgp[i]:
                    fd[i] -= slp[i]
                    slp[i] = 0
                elif fgp[i] == 1 and not fd[i]:
                    fgp[i] -= slp[i]
                    slp[i] = 0
                    sgp += 1
        for i in range(l):
            if sgp >= fd[i]:
                sgp -= fd[i]
            else:
                return False
        return True


class OptLRC(_MixedLRC):
    pass


class UniCauLRC(_MixedLRC):
    pass


class OptCauLRC(AzureLRC):
    """Groups as Azure; a local parity also covers the global parities (lrc.cpp:1485-1518)."""

    surviving_group_id = 0  # lrc.h:171, uninitialised in the reference (only read after being set)

    def partition_sub_optimal(self):
        raise ValueError("sub-optimal placement is Azure-only")

    def check_if_decodable(self, fs):  # lrc.cpp:1415-1483
        k, l, g, r = self.k, self.l, self.g, self.r
        fd, slp, sgp, fdc = [0] * l, [1] * l, g, 0
        for b in fs:
            if b < k:
                fd[b // r] += 1
                fdc += 1
            elif b < k + g:
                sgp -= 1
            else:
                slp[b - k - g] -= 1
        if sgp < g:
            healthy = sum(1 for i in range(l) if slp[i] and not fd[i])
            if healthy >= g - sgp:
                sgp = g
        if sgp < g:
            return sgp >= fdc
        for i in range(l):
            if slp[i] and slp[i] <= fd[i]:
                fd[i] -= slp[i]
                slp[i] = 0
        for i in range(l):
            if sgp >= fd[i]:
                sgp -= fd[i]
            else:
                return False
        return True

    def help_single(self, fi):  # lrc.cpp:1757-1859
        k, g = self.k, self.g
        if not self.partition_plan:
            return []
        if not self.local_or_column:
            return super().help_single(fi)
        out = []
        glob = lambda b: k <= b < k + g  # noqa: E731
        for p in self.partition_plan:
            if glob(fi):
                h = [b for b in p if (glob(b) and b != fi) or self.bid2gid(b) == self.surviving_group_id]
            else:
                gid = self.bid2gid(fi)
                h = [b for b in p if (self.bid2gid(b) == gid and b != fi) or glob(b)]
            if h:
                out.append(h)
        return out

    def generate_repair_plan(self, fs):  # lrc.cpp:1861-2023
        k, l, g = self.k, self.l, self.g
        n = k + g + l
        if not self.check_if_decodable(fs):
            return False, []
        plans = []
        if len(fs) == 1:
            self.local_or_column = True
            plans.append(RepairPlan(True, list(fs), self.help_single(fs[0])))
            return True, plans
        failed = [0] * n
        gc = [0] * (l + 1)
        ndg, nf = 0, len(fs)
        for f in fs:
            failed[f] = 1
            gc[self.bid2gid(f)] += 1
            if f < k + g:
                ndg += 1
                if f >= k:
                    for j in range(l):
                        gc[j] += 1
        it = 0
        while nf > 0:
            for i in range(n):
                if k <= i < k + g and failed[i]:
                    for j in range(l):
                        if gc[j] == 1:
                            self.local_or_column = True
                            self.surviving_group_id = j
                            plans.append(RepairPlan(True, [i], self.help_single(i)))
                            failed[i] = 0
                            for jj in range(l + 1):
                                gc[jj] -= 1
                            nf -= 1
                            ndg -= 1
                            break
            for gid in range(l):
                if gc[gid] == 1:
                    cand = [i for i in range(n) if failed[i] and self.bid2gid(i) == gid]
                    if not cand:
                        continue
                    fi = cand[0]
                    self.local_or_column = True
                    plans.append(RepairPlan(True, [fi], self.help_single(fi)))
                    failed[fi] = 0
                    gc[gid] = 0
                    nf -= 1
                    if fi < k + g:
                        ndg -= 1
            if 0 < ndg <= g:
                p = RepairPlan(False, [i for i in range(k + g) if failed[i]], [])
                if len(p.failure_idxs) == 1:
                    self.local_or_column = False
                    p.help_blocks = self.help_single(p.failure_idxs[0])
                else:
                    p.help_blocks = self.help_multi(p.failure_idxs)
                plans.append(p)
                for i in range(k + g):
                    if failed[i]:
                        failed[i] = 0
                        nf -= 1
                        gc[self.bid2gid(i)] -= 1
                        if i >= k:
                            for j in range(l):
                                gc[j] -= 1
                ndg = 0
            if it > 0 and nf > 0:
                if not self.check_if_decodable(fs):
                    return False, plans
                p = RepairPlan(False, [i for i in range(n) if failed[i]], [])
                p.help_blocks = self.help_multi(p.failure_idxs)
                plans.append(p)
                for i in range(n):
                    if failed[i]:
                        failed[i] = 0
                        nf -= 1
                        gc[self.bid2gid(i)] -= 1
                        if k <= i < k + g:
                            for j in range(l):
                                gc[j] -= 1
                ndg = 0
            it += 1
        return True, plans


class PC(Planner):
    with_global = True

    def __init__(self, k1, m1, k2, m2):  # pc.h:21-24
        k = k1 * k2
        m = (k1 + m1) * (k2 + m2) - k if self.with_global else k1 * m2 + k2 * m1
        super().__init__(k, m)
        self.k1, self.m1, self.k2, self.m2 = k1, m1, k2, m2
        self.row_code = RS(k1, m1)

    def rowcol2bid(self, row, col):  # pc.cpp:326-340
        k1, m1, k2 = self.k1, self.m1, self.k2
        if row < k2 and col < k1:
            return row * k1 + col
        if row < k2:
            return k1 * k2 + row * m1 + (col - k1)
        if col < k1:
            return (k1 + m1) * k2 + (row - k2) * k1 + col
        return (k1 + m1) * k2 + k1 * self.m2 + (row - k2) * m1 + (col - k1)

    def bid2rowcol(self, bid):  # pc.cpp:342-359
        k1, m1, k2 = self.k1, self.m1, self.k2
        if bid < k1 * k2:
            return bid // k1, bid % k1
        if bid < (k1 + m1) * k2:
            t = bid - k1 * k2
            return t // m1, t % m1 + k1
        if bid < (k1 + m1) * k2 + k1 * self.m2:
            t = bid - (k1 + m1) * k2
            return t // k1 + k2, t % k1
        t = bid - (k1 + m1) * k2 - k1 * self.m2
        return t // m1 + k2, t % m1 + k1

    def _column(self, col):
        rows = self.k2 + self.m2 if (col < self.k1 or self.with_global) else self.k2
        return [self.rowcol2bid(r, col) for r in range(rows)]

    def partition_flat(self):  # pc.cpp:378-388
        self.row_code.partition_plan = [[i] for i in range(self.k1 + self.m1)]
        self.partition_plan += [[i] for i in range(self.k + self.m)]

    def partition_random(self):  # pc.cpp:390-421 / 1091-1129
        self.row_code.partition_plan = []
        n = self.k1 + self.m1
        cols = list(range(n))
        cnt = 0
        while cnt < n:
            nc = min(self.random_range(1, self.m1), n - cnt)
            part, rp = [], []
            for _ in range(nc):
                c = cols.pop(self.random_index(n - cnt))
                cnt += 1
                part += self._column(c)
                rp.append(c)
            self.partition_plan.append(part)
            self.row_code.partition_plan.append(rp)

    def partition_optimal(self):  # pc.cpp:423-443 / 1131-1158
        self.row_code.partition_plan = []
        n = self.k1 + self.m1
        for s in range(0, n, self.m1):
            cs = list(range(s, min(n, s + self.m1)))
            self.partition_plan.append([b for c in cs for b in self._column(c)])
            self.row_code.partition_plan.append(cs)

    def partition_sub_optimal(self):
        raise ValueError("sub-optimal placement is Azure-only")

    def generate_repair_plan(self, fs):  # pc.cpp:451-551 / HVPC 1166-1264
        k1, m1, k2, m2 = self.k1, self.m1, self.k2, self.m2
        R, C = k2 + m2, k1 + m1
        ncols, nrows = (C, R) if self.with_global else (k1, k2)
        fmap = [[0] * C for _ in range(R)]
        frc, fcc = [0] * R, [0] * C
        for b in fs:
            r, c = self.bid2rowcol(b)
            fmap[r][c] = 1
            frc[r] += 1
            fcc[c] += 1
        nf = len(fs)
        plans = []
        while nf > 0:
            for i in range(ncols):
                if 0 < fcc[i] <= m2:
                    p = RepairPlan(True, [], [])
                    help_, cnt = [], 0
                    for jj in range(R):
                        if cnt == k2:
                            break
                        if not fmap[jj][i]:
                            help_.append(self.rowcol2bid(jj, i))
                            cnt += 1
                    p.help_blocks = [[b] for b in help_] if self.placement_rule == FLAT else [help_]
                    for jj in range(R):
                        if fmap[jj][i]:
                            p.failure_idxs.append(self.rowcol2bid(jj, i))
                            fmap[jj][i] = 0
                            nf -= 1
                            frc[jj] -= 1
                            fcc[i] -= 1
                    plans.append(p)
            if nf == 0:
                break
            max_row = -1
            for i in range(nrows):
                if 0 < frc[i] <= m1:
                    max_row = i
                    cols = [jj for jj in range(C) if fmap[i][jj]]
                    hb = self.row_code.help_multi(cols)
                    p = RepairPlan(False, [], [[self.rowcol2bid(i, c) for c in h] for h in hb])
                    for jj in range(C):
                        if fmap[i][jj]:
                            p.failure_idxs.append(self.rowcol2bid(i, jj))
                            fmap[i][jj] = 0
                            nf -= 1
                            frc[i] -= 1
                            fcc[jj] -= 1
                    plans.append(p)
                    break
            if max_row == -1:
                return False, plans
        return True, plans


class HVPC(PC):
    with_global = False


def planner_for(name, params):
    """name: the ECTYPE member name used by tests/golden (RS, ERS, AZURE_LRC, ...)."""
    if name in ("RS", "ERS"):
        return RS(params["k"], params["m"])
    if name in ("PC", "Hierachical_PC"):
        return PC(params["k1"], params["m1"], params["k2"], params["m2"])
    if name == "HV_PC":
        return HVPC(params["k1"], params["m1"], params["k2"], params["m2"])
    cls = {"AZURE_LRC": AzureLRC, "AZURE_LRC_1": AzureLRC1, "OPTIMAL_LRC": OptLRC,
           "OPTIMAL_CAUCHY_LRC": OptCauLRC, "UNIFORM_CAUCHY_LRC": UniCauLRC}[name]
    return cls(params["k"], params["l"], params["g"])
