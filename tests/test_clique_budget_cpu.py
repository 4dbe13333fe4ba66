"""CPU (-m "not gpu") half of the clique kernel's exhausted-budget tests: the model (clique_budget_model.py) against the oracle and
the live networkx, the properties of its answers over the budgets, the conditions the cases (clique_budget_cases.py) were picked
for, and the two mutants that show that the listed (case, budget) pairs see the budget test's place and the matching bound.
The GPU half is test_gpu_clique_budget.py."""
import numpy as np
import pytest

import oracle
import clique_budget_cases as cases
import clique_budget_model as model


def _is_clique(c, mask):
    members = [u for u in range(c.K) if (mask >> u) & 1]
    return all((c.rows[u] & mask) == mask & ~(1 << u) for u in members)


def test_model_without_budget_is_the_oracle_and_the_live_networkx():
    for c in cases.all_cases():
        mask, n, proven, n1, n2 = c.full
        size, omask, _ = oracle.max_clique_nx(c.adj_words)
        assert proven and n == size and np.array_equal(model.mask_array(mask, c.K), omask), c.name
        assert n2 >= n1, c.name
    nx = pytest.importorskip("networkx")
    live = 0
    for c in cases.all_cases():
        if c.K > 140:
            continue
        A = oracle.adjacency_dense(c.adj_words, c.K)
        G = nx.Graph((A | np.eye(c.K, dtype=bool)).astype(np.int8))
        best = []
        for q in nx.find_cliques(G):
            if len(q) > len(best):
                best = q
        want = np.zeros(c.K, bool)
        want[np.array(best, int)] = True
        assert np.array_equal(c.mask_array(0), want), c.name
        live += 1
    assert live >= 8, live


def test_phase_1_does_not_depend_on_the_budget_once_it_fits():
    for c in cases.all_cases():
        wit = c.witness()
        for L in c.budgets:
            mask, n, proven, n1, n2 = c.run(L)
            if L == 0 or L >= c.n1:
                assert n1 == c.n1, (c.name, L)
                if 0 < L < c.n2:
                    assert not proven and mask == wit and n2 == L + 1, (c.name, L)      # cut inside the walk: exactly the witness
                else:
                    assert proven and mask == c.full[0] and n2 == c.n2, (c.name, L)
            else:
                assert not proven and n1 == n2 == L + 1, (c.name, L)                    # cut inside phase 1, at node L + 1


def test_every_mask_is_a_clique_that_grows_with_the_budget():
    for c in cases.all_cases():
        omega = c.full[1]
        last = 0
        for L in [b for b in c.budgets if b] + [0]:                                    # ascending, the default budget last
            mask, n, proven, _, _ = c.run(L)
            assert n == bin(mask).count("1") and _is_clique(c, mask), (c.name, L)
            assert n >= last, (c.name, L)
            last = n
            if L == 0 or L >= c.n1:
                assert n == omega, (c.name, L)
        # the budget of the first non-empty mask is that: empty just below it
        assert c.run(c.first)[1] > 0, c.name
        if c.first > 1:
            assert c.run(c.first - 1)[1] == 0, c.name


def test_case_conditions():
    cs = cases.all_cases()
    sizes = {c.K for c in cs if c.name.startswith("tie")}
    assert {64, 65, 128, 129} <= sizes and min(sizes) == 20 and max(sizes) == 320
    assert any(c.K * ((c.K + 63) // 64) > 8192 for c in cs)                            # CQ_LDS_ADJ_WORDS: adjacency read from global memory
    assert {"real95", "tiny02", "tiny08"} <= {c.name for c in cs}
    walk = [c.name for c in cs if c.n2 > c.n1]
    differ = [c.name for c in cs if c.witness() != c.full[0]]
    empty = [c.name for c in cs if any(L >= 1 and c.run(L)[1] == 0 for L in c.budgets)]
    past = [c.name for c in cs if c.n1 > model.MATCH_AFTER]
    print("cases", len(cs), "| (case, budget) pairs", sum(len(c.budgets) for c in cs))
    print("n1 / n2 / first non-empty:", {c.name: (c.n1, c.n2, c.first) for c in cs})
    print("n2 > n1:", len(walk), walk)
    print("witness differs from the networkx mask:", len(differ), differ)
    print("an empty mask at some L >= 1:", len(empty), empty)
    print("n1 > %d:" % model.MATCH_AFTER, len(past), past)
    assert all(c.n1 >= 2 for c in cs), [(c.name, c.n1) for c in cs]
    assert 2 * len(walk) >= len(cs)
    assert 3 * len(differ) >= len(cs)
    assert len(empty) >= 1 and len(past) >= 1
    assert set(cases.ONE_WAVE_CASES) <= {c.name for c in cs} and 3 * len(cases.ONE_WAVE_CASES) >= len(cs)
    for c in cs:
        want = {1, 2, 3, c.first, c.n1 - 1, c.n1, c.n1 + 1, (c.n1 + c.n2) // 2, c.n2 - 1, c.n2, c.n2 + 1}
        assert set(c.budgets) == {L for L in want if L >= 1} | {0}, c.name


@pytest.mark.parametrize("mutant", model.MUTANTS)
def test_the_listed_budgets_see_the_rule(mutant):
    """the model with the budget test moved before the count, and with the matching bound left out, answers another (n, proven) on
    at least one listed (case, budget): a kernel with that rule wrong fails the GPU table"""
    hits = []
    for c in cases.all_cases():
        if mutant == "no_matching_bound" and c.n2 <= model.MATCH_AFTER:
            continue                                                                  # (the bound never runs there: nothing to see)
        for L in c.budgets:
            got = model.run(c.rows, c.K, L, mutant=mutant)
            if (got[1], got[2]) != c.run(L)[1:3]:
                hits.append((c.name, L))
    print(mutant, "seen at", hits)
    assert hits, mutant


def test_engine_budget_covers_every_row_of_the_table():
    """ENGINE_LIMIT against the three lanes of the engine test, tracked by the oracle: one lane-step at least is cut inside phase 1,
    one inside the walk, one stays proven"""
    steps = cases.engine_lane_steps(cases.ENGINE_LIMIT)
    print("engine lane-steps (step, lane, n_good, n_inliers, proven, regime) at L =", cases.ENGINE_LIMIT, steps)
    assert {"cut", "witness", "proven"} <= {s[5] for s in steps}
    for _, _, _, _, proven, reg in steps:
        assert proven == (reg == "proven")
