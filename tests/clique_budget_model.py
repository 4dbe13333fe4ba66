"""max_clique_kernel (csrc/clique.hip) when its node budget runs out: a plain-Python restatement of what decides the answer.

The kernel counts search nodes in CqCtx.nodes across every call of cq_solve and gives up once the count passes node_limit: bit 0 of
flags ("proven") goes to 0 and the mask is whatever REC holds.  With n1 = the nodes of phase 1 (cq_solve on the whole graph) and
n2 >= n1 = the total including the walk's existence queries:

    L <  n1        unproven, phase 1's best so far (REC is assigned at a completed maximal clique only: empty before the first leaf)
    n1 <= L < n2   unproven, exactly phase 1's witness (REC = WIT is copied before the walk; the walk's WIT = QB | RQ never reaches it)
    L >= n2        proven, networkx's first strictly-largest clique

solve() is cq_solve statement for statement; bitsets are Python ints.  run() is the kernel's body: phase 1, the unique-core check
(no nodes, but it decides whether the walk runs), and nx_walk at the logical level - pivot, ext_u, pop, cand.remove, subg & adj[q],
cand & adj[q] on CPython's own sets, as networkx.find_cliques writes them (the kernel restates CPython's set;
tests/test_oracle_clique_order.py pins that restatement to the live interpreter) - with the kernel's shortcuts and its calls of
cq_solve exactly where the kernel makes them.  Counts (|cand & adj[u]|, |subg & adj[q]|) are taken from bit mirrors of the sets;
every ORDER (pivot ties, pop) comes from the sets themselves.

nx_bulk has no counterpart here, and needs none: it only skips forced levels.  A vertex of cand adjacent to all the rest of cand
belongs to every maximum clique of the subtree, so it is in the witness, the witness test answers for it and no query is made on
such a level - with or without the bulk the same queries are asked in the same order, and the same leaf is reached.

mutant = NAME (one of MUTANTS) changes one rule; only there so that the CPU test can show that the listed (case, budget) pairs
see that rule (tests/test_clique_budget_cpu.py).
"""
DEFAULT_NODE_LIMIT = 300000     # launch_max_clique: node_limit <= 0
MATCH_AFTER = 256               # CQ_MATCH_AFTER
NO_TARGET = 0x7fffffff

MUTANTS = ("budget_test_before_count", "no_matching_bound")


class Ctx:
    """CqCtx: the adjacency rows and what runs on across calls of solve()"""

    def __init__(self, adj, K, limit, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.adj, self.K = adj, K
        self.nodes = 0
        self.limit = limit if limit > 0 else DEFAULT_NODE_LIMIT
        self.complete = True
        self.mutant = mutant
        self.first_rec_nodes = None                                 # (the model's own note) the count at which REC was first assigned


def _bits(x):
    while x:
        b = x & -x
        yield b.bit_length() - 1, b
        x ^= b


def solve(ctx, P0, best, target, rec=0):
    """cq_solve: the size of a maximum clique inside P0 if it exceeds `best` (else `best`), stopping at `target` -> (best, REC).
    REC is the caller's `rec` until a maximal clique improves on `best`."""
    A = ctx.adj
    P, R, size = P0, 0, 0
    stack = []                                                      # levels: [P, R, size, v, stage]
    pending = True
    while True:
        if pending:
            pending = False
            vbr, dead = -1, False
            while True:                                             # reductions to a fixed point
                cnt = P.bit_count()
                if size + cnt <= best:
                    dead = True
                    break
                if cnt == 0:
                    break
                thr = best - size
                RM = UN = PE = 0
                key = NO_TARGET
                for u, b in _bits(P):                               # cq_degrees
                    d = (A[u] & P).bit_count()
                    if d < thr:
                        RM |= b
                    if d == cnt - 1:
                        UN |= b
                    if d == cnt - 2:
                        PE |= b
                    key = min(key, d * 2048 + (2047 - u))
                if RM:
                    P &= ~RM
                    continue
                if UN:
                    R |= UN
                    size += UN.bit_count()
                    P &= ~UN
                    continue
                if PE:                                              # all pendants of this pass, ascending, with their partners
                    for pv, bv in _bits(PE):
                        if not P & bv:
                            continue
                        rest = P & ~A[pv] & ~bv
                        R |= bv
                        size += 1
                        P &= ~bv
                        if rest:
                            P &= ~(rest & -rest)
                    continue
                vbr = 2047 - (key & 2047)
                break
            if dead:
                continue
            if P == 0:                                              # a maximal clique of this branch
                if size > best:
                    best, rec = size, R
                    if ctx.first_rec_nodes is None:
                        ctx.first_rec_nodes = ctx.nodes
                    if best >= target:
                        return best, rec
                continue
            if ctx.mutant == "budget_test_before_count":
                if ctx.nodes > ctx.limit:
                    ctx.complete = False
                    return best, rec
                ctx.nodes += 1
            else:
                ctx.nodes += 1
                if ctx.nodes > ctx.limit:
                    ctx.complete = False
                    return best, rec
            if ctx.nodes > MATCH_AFTER and ctx.mutant != "no_matching_bound":      # greedy matching bound on the conflict graph of P
                Q = P
                slack = size + P.bit_count() - best
                pruned = False
                while Q:
                    bv = Q & -Q
                    v = bv.bit_length() - 1
                    rest = Q & ~A[v] & ~bv
                    Q &= ~bv
                    if not rest:
                        continue
                    Q &= ~(rest & -rest)
                    slack -= 1
                    if slack <= 0:
                        pruned = True
                        break
                if pruned:
                    continue
            stack.append([P, R, size, vbr, 0])
            continue
        if not stack:
            return best, rec
        lvl = stack[-1]
        Pl, Rl, sl, v, stage = lvl
        if stage >= 2:
            stack.pop()
            continue
        lvl[4] = stage + 1
        if sl + Pl.bit_count() <= best:
            stack.pop()
            continue
        bv = 1 << v
        if stage == 0:                                              # without the most conflicting vertex
            P, R, size = Pl & ~bv, Rl, sl
        else:                                                       # with it: its conflicts leave
            P, R, size = Pl & A[v], Rl | bv, sl + 1
        pending = True


def walk(ctx, omega, WIT):
    """nx_walk: (True, the first clique of size omega in networkx.find_cliques order) or (False, _) when a query ran out of nodes"""
    A, K = ctx.adj, ctx.K
    adj = []
    for u in range(K):                                              # adj = {u: {v for v in G[u] if v != u}}: ascending insertion
        s = set()
        for v, _ in _bits(A[u]):
            s.add(v)
        adj.append(s)
    cand = set(range(K))                                            # set(G)
    subg = cand.copy()
    candb = subgb = (1 << K) - 1
    RF, size = 0, 0
    entered = True
    ext_u = None
    while True:
        if entered:
            entered = False
            if len(cand) == omega - size:
                return True, RF | candb
            u = max(subg, key=lambda u: (candb & A[u]).bit_count())  # len(cand & adj[u]); the first maximum in subg's order
            ext_u = cand - adj[u]
        if not ext_u:
            return False, RF                                        # cannot happen while the existence answers are exact
        q = ext_u.pop()
        cand.remove(q)
        bq = 1 << q
        candb &= ~bq
        Sq, Cq = subgb & A[q], candb & A[q]
        s1 = size + 1
        if not Sq:                                                  # maximal clique Q + q
            if s1 >= omega:
                return True, RF | bq
            continue
        ncq = Cq.bit_count()
        if ncq == 0:
            continue
        need = omega - s1
        if need <= 0:
            return True, RF | bq
        if ncq < need:
            continue
        QB = RF | bq
        ok = not (QB & ~WIT) and not (WIT & ~QB & ~Cq)              # the witness lives in this subtree
        if not ok:
            got, RQ = solve(ctx, Cq, need - 1, need)
            if not ctx.complete:
                return False, RF
            if got >= need:
                ok = True
                WIT = QB | RQ
        if not ok:
            continue
        if ncq == need:
            return True, QB | Cq
        subg = subg & adj[q]
        cand = cand & adj[q]
        subgb, candb = Sq, Cq
        RF, size = QB, s1
        entered = True


def run(adj, K, limit, mutant=None):
    """max_clique_kernel on K vertices with adjacency rows adj[u] (Python ints, no self loops) and node_limit = limit
    -> (mask as an int, n_inliers, proven, n1, n2): n1 = the nodes counted when phase 1 returned, n2 = when the kernel did"""
    ctx = Ctx(adj, K, limit, mutant)
    ALL = (1 << K) - 1
    omega, WIT = solve(ctx, ALL, 0, NO_TARGET)
    n1 = ctx.nodes
    REC = WIT
    unique = False
    if ctx.complete and omega > 1:                                  # a (omega - 1)-core of exactly omega vertices is the only maximum clique
        P = ALL
        while True:
            cnt = P.bit_count()
            if cnt <= omega:
                unique = cnt == omega
                break
            RM = 0
            for u, b in _bits(P):
                if (adj[u] & P).bit_count() < omega - 1:
                    RM |= b
            if not RM:
                break
            P &= ~RM
    if ctx.complete and omega > 0 and not unique:
        ok, RF = walk(ctx, omega, WIT)
        if ok:
            REC = RF
    return REC, REC.bit_count(), ctx.complete, n1, ctx.nodes


def first_nonempty_budget(adj, K):
    """the smallest node_limit >= 1 at which the mask is not empty: REC first assigned with m nodes counted survives every cut at a
    later node, i.e. every L >= m.  (A hint for choosing budgets; the CPU test runs the budgets on either side of it.)"""
    ctx = Ctx(adj, K, 0)
    solve(ctx, (1 << K) - 1, 0, NO_TARGET)
    return max(1, ctx.first_rec_nodes)


def rows_from_words(adj_words, K):
    """oracle.consistency_graph's (K, nw) uint64 rows -> the list of Python ints run() takes"""
    return [int.from_bytes(adj_words[u].tobytes(), "little") & ((1 << K) - 1) for u in range(K)]


def mask_array(mask, K):
    import numpy as np
    return np.array([(mask >> u) & 1 for u in range(K)], bool)
