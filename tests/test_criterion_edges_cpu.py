"""The edge cases of tests/criterion_edges_ref.py are sound before any kernel sees them (no GPU): every case carries the edge it is named
for; the fp64 references are finite and the closed form equals autograd to 1e-12; eight times the fp32 floor stays at or under the bars
the golden tests use (a cap on the inputs, not a measurement: a case that breaks it gets other inputs); every mutant of the closed form
moves the tensor CATCHES names by more than ten bars, and every edge case catches one; the +-2 ulp bracket of the match cost contains the
fp32 oracle, has zero width from logit 20 up, and the duplicate-target assignments are decided by more than the bracket widths."""
import numpy as np
import pytest
import torch

import criterion_edges_ref as R
from oracle import criterion as OC
from oracle import lsap as oracle_lsap

case_param = pytest.mark.parametrize("name", R.CASES)
match_param = pytest.mark.parametrize("launch,table", R.MATCH_CASES, ids=[f"{a}-{b}" for a, b in R.MATCH_CASES])
TENSORS = R.SCALARS + R.GRADS


def xyxy(box):
    cx, cy, w, h = (float(v) for v in box)
    return cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h


def pairs_of(c, mark):
    out = [c.pair(b, k) for b, k in c.marks[mark]]
    assert out, mark
    return [(xyxy(p), xyxy(t), p, t) for p, t in out]


def test_every_case_is_dyadic_with_valid_ascending_indices():
    cases = [R.case(n) for n in R.CASES] + [R.size_case(B, Q) for B, Q in R.SIZE_CASES[:1]]
    for c in cases:
        for t in [c.boxes.reshape(-1, 4)] + c.tgt_boxes:
            assert torch.equal(t * 64, (t * 64).round()) and bool((t[:, 2:] >= 1 / 64).all()), c.name
        assert bool((c.vars > 0).all()) and bool(torch.isfinite(c.logits).all())
        assert c.B in (1, 2, 3, 64) and c.Q in (24, 40)
        for b, (i, j) in enumerate(c.idx):
            T = c.sizes[b]
            assert len(i) == len(j) == min(c.Q, T)
            assert bool((i[1:] > i[:-1]).all()) and len(set(j.tolist())) == len(j)
            assert (len(i) == 0) or (0 <= int(i.min()) and int(i.max()) < c.Q and 0 <= int(j.min()) and int(j.max()) < T)
            assert bool(((c.tgt_labels[b] >= 0) & (c.tgt_labels[b] < c.num_classes)).all())
        ii, jj = R.device_indices(c)                       # padded slots: in range, and not the image's own pair
        assert int(ii.min()) >= 0 and int(ii.max()) < c.Q and int(jj.min()) >= 0
        for b, (i, _) in enumerate(c.idx):
            assert bool((ii[b, len(i):] == c.Q - 1).all()) and bool((jj[b, len(i):] == 0).all())
    assert {(R.case(n).logits.shape[2], R.case(n).num_classes) for n in R.CASES} == {(2, 1), (3, 3)}
    assert {R.case(n).B for n in R.CASES} == {1, 2, 3} and {R.case(n).Q for n in R.CASES} == {24, 40}


def test_box_cases_carry_their_edges_in_fp32():
    f = np.float32
    for (x1, y1, x2, y2), (u1, v1, u2, v2), p, t in pairs_of(R.case("identical"), "identical"):
        assert (x1, y1, x2, y2) == (u1, v1, u2, v2) and [float(v) for v in (p - t)] == [0.0] * 4         # four zero residuals, every max / min a tie
    for (x1, y1, x2, y2), (u1, v1, u2, v2), _, _ in pairs_of(R.case("shared_edge"), "touch_x"):
        assert f(min(x2, u2)) - f(max(x1, u1)) == 0.0 and min(y2, v2) - max(y1, v1) > 0                  # iw0 == 0 with a positive overlap in y
        assert len({y1, y2, v1, v2}) == 4
    for (x1, y1, x2, y2), (u1, v1, u2, v2), _, _ in pairs_of(R.case("shared_edge"), "touch_y"):
        assert f(min(y2, v2)) - f(max(y1, v1)) == 0.0 and min(x2, u2) - max(x1, u1) > 0
    inner = 0
    for (x1, y1, x2, y2), (u1, v1, u2, v2), p, t in pairs_of(R.case("concentric"), "concentric"):
        assert float(p[0]) == float(t[0]) and float(p[1]) == float(t[1])
        assert (u1 < x1 and x2 < u2 and v1 < y1 and y2 < v2) or (x1 < u1 and u2 < x2 and y1 < v1 and v2 < y2)
        inner += u1 < x1
    assert inner >= 1                                                                                    # a prediction inside its target
    for (x1, y1, x2, y2), (u1, v1, u2, v2), p, t in pairs_of(R.case("same_cx_w"), "same_cx_w"):
        assert x1 == u1 and x2 == u2 and len({y1, y2, v1, v2}) == 4 and float(p[1]) != float(t[1])       # ties in x only
    for (x1, y1, x2, y2), (u1, v1, u2, v2), _, _ in pairs_of(R.case("disjoint"), "disjoint"):
        enclosing = (max(x2, u2) - min(x1, u1)) * (max(y2, v2) - min(y1, v1))
        assert min(x2, u2) < max(x1, u1) and min(y2, v2) < max(y1, v1)
        assert enclosing > 10 * ((x2 - x1) * (y2 - y1) + (u2 - u1) * (v2 - v1))                          # much larger than the union
    small = [min(float(p[2]), float(t[2])) for _, _, p, t in pairs_of(R.case("tiny"), "tiny")]
    assert small == [1 / 64] * len(small)


def test_logit_variance_and_count_cases_carry_their_edges():
    c = R.case("logit_sat")
    matched = torch.stack([c.logits[b, c.idx[b][0][k]] for b, k in c.marks["sat_matched"]])
    unmatched = torch.stack([c.logits[b, q] for b, q in c.marks["sat_unmatched"]])
    for col in (matched[:10, 0], matched[10:, 1], unmatched[:, 0], unmatched[:, 1]):
        assert sorted(col.tolist()) == sorted(R.SAT)
    assert not any(bool(R.matched_rows(c)[b, q]) for b, q in c.marks["sat_unmatched"] + c.marks["tie_unmatched"])
    ties = [tuple(c.logits[b, c.idx[b][0][k]].tolist()) for b, k in c.marks["tie_matched"]]
    assert sorted(ties) == sorted(R.TIES) == sorted(tuple(c.logits[b, q].tolist()) for b, q in c.marks["tie_unmatched"])
    v = R.case("var_edges")
    got = torch.cat([v.vars[b, v.idx[b][0]].reshape(-1) for b in range(v.B)])
    assert set(got.tolist()) == {float(torch.tensor(x, dtype=torch.float32)) for x in R.VAR_EDGES}
    assert float(torch.tensor(1.0).log()) == 0.0 and 1.0 in got.tolist()                                  # sign(log v) at v == 1
    t = R.case("t_gt_q")
    assert t.sizes[0] == t.Q + 5 and t.idx[0][0].tolist() == list(range(t.Q))                            # every query matched ...
    assert sorted(t.idx[0][1].tolist()) != list(range(t.Q))                                              # ... and idx_j is no prefix of the targets
    m = R.case("t_mixed")
    assert m.sizes == (9, 0, 1) and tuple(R.device_indices(m)[0].shape) == (3, 9)
    n = R.case("t_none")
    assert n.sizes == (0, 0) and tuple(R.device_indices(n)[0].shape) == (2, 1)
    assert R.reference(n)["class_error"] == 100.0 and R.reference(n)["loss_bbox"] == 0.0
    k3 = R.case("c3")
    assert set(torch.cat(k3.tgt_labels).tolist()) == {0, 1, 2}


@case_param
def test_reference_is_finite_and_the_closed_form_is_autograd(name):
    c = R.case(name)
    ref, cf = R.reference(c), R.closed_form(c)
    for k in TENSORS:
        assert bool(torch.isfinite(torch.as_tensor(ref[k])).all()), k
        assert R.err(k, cf[k], ref[k]) <= 1e-12, (k, R.err(k, cf[k], ref[k]))
    for k in R.EXACT:
        assert cf[k] == ref[k]
    parts = ((("d_logits/ce", R.W6[0]),), (("d_boxes/bbox", R.W6[3]), ("d_boxes/giou", R.W6[4]), ("d_boxes/var", R.W6[5])), (("d_vars/var", R.W6[5]),))
    for i, part in enumerate(parts):                                                                     # the per-loss gradients add up to the total's
        assert R.err("d_vars" if i == 2 else "d_total", sum(w * ref[k] for k, w in part), ref["d_total"][i]) <= 1e-12
    rows = R.matched_rows(c)
    for k in R.GRADS[1:]:                                                                                # unmatched queries: exactly 0
        assert float(ref[k][~rows].abs().sum()) == 0.0
    for b in range(c.B):
        per = R.reference_per_image(c, b)
        assert all(np.isfinite(per[k]) for k in R.SCALARS)
        if c.sizes[b] == 0:
            assert per["class_error"] == 100.0 and per["loss_bbox"] == per["loss_giou"] == per["loss_variance"] == 0.0


@pytest.mark.parametrize("name", R.CASES + tuple(f"size_b{B}_q{Q}" for B, Q in R.SIZE_CASES))
def test_eight_floors_stay_under_the_existing_bars(name):
    """The cap: with 8 x floor <= the golden tests' bars, min(existing, max(8 x floor, 2^-21)) is never looser than today's check."""
    c = R._lookup(name)
    fl = R.floor(c)
    for k, v in fl.items():
        cap = R.EXISTING["scalar"] if k in R.SCALARS else R.EXISTING["grad"]
        print(f"FLOOR {name} {k}: {v:.2e}")
        assert R.FACTOR * v <= cap, (k, v)
        assert k not in R.EXACT or v == 0.0
    if not name.startswith("size_"):
        for b in range(c.B):
            for k, v in R.floor_per_image(c, b).items():
                if k in R.SCALARS:
                    assert R.FACTOR * v <= R.EXISTING["scalar"], (b, k, v)


def moved_by(c, mutant, tensor):
    ref = R.reference(c)
    return R.err(tensor, R.closed_form(c, **R.MUTANTS[mutant])[tensor], ref[tensor])


def test_every_mutant_is_caught_where_the_table_says():
    assert set(R.CATCHES) == set(R.MUTANTS)
    for mutant, where in R.CATCHES.items():
        assert where
        for name, tensor in where:
            c = R.case(name)
            b = R.bar(R.existing(tensor), R.floor(c)[tensor])
            moved = moved_by(c, mutant, tensor)
            print(f"MUTANT {mutant}: {name} {tensor} moved {moved:.2e}, bar {b:.2e}")
            assert moved > 10 * b, (mutant, name, tensor, moved, b)
    caught_by = {name for where in R.CATCHES.values() for name, _ in where}
    assert caught_by == set(R.CASES), set(R.CASES) - caught_by                                           # every edge case catches a mutant


def test_the_edge_is_what_catches_the_clamp_and_argmax_mutants():
    """A case without touching boxes or tied logits does not see these mutants at all, bit for bit: it takes none of their branches."""
    plain, right = R.case("disjoint"), R.closed_form(R.case("disjoint"))
    for mutant in ("clamp_strict", "argmax_last"):
        wrong = R.closed_form(plain, **R.MUTANTS[mutant])
        for k in TENSORS:
            assert torch.equal(torch.as_tensor(wrong[k]), torch.as_tensor(right[k])), (mutant, k)


# ----------------------------------------------------------------------------------------------------- match cost
def test_match_tables_cover_what_they_claim():
    assert R.MATCH_LAUNCHES["sizes"] == (17, R.MATCH_Q, 45) and R.MATCH_LAUNCHES["few"] == (1, 0, 12)
    p = R.match_case("sizes", "pinned").logits[..., 0]
    free = torch.ones_like(p, dtype=torch.bool)
    free[:, 10:18], free[:, 0] = False, False
    assert float(p[free].abs().max()) <= 2.0 and sorted(p[0, 10:18].tolist()) == sorted(R.PINNED_SAT) and float(p[0, 0]) == 20.0
    b = R.match_case("sizes", "band").logits[..., 0]
    assert float(b.min()) == 4.5 and float(b.max()) == 17.0
    s = R.match_case("sizes", "golden_scale").logits[..., 0]
    assert 2.0 < float(s.std()) < 4.0 and float(s.max()) > 6 and float(s.min()) < -6
    for launch, table in R.MATCH_CASES:
        mc = R.match_case(launch, table)
        q, q2 = mc.dup_q
        assert torch.equal(mc.boxes[:, q], mc.boxes[:, q2]) and torch.equal(mc.logits[:, q], mc.logits[:, q2])
        for bb, (j, j2) in mc.dup_t.items():
            assert torch.equal(mc.tgt[bb][j], mc.tgt[bb][j2])
        assert set(mc.dup_t) == {bb for bb, t in enumerate(mc.sizes) if t >= 9}
        for t in [mc.boxes.reshape(-1, 4)] + mc.tgt:
            assert torch.equal(t * 64, (t * 64).round()) and bool((t[:, 2:] >= 1 / 64).all())


@match_param
def test_match_oracle_is_finite_and_inside_its_bracket(launch, table):
    mc = R.match_case(launch, table)
    for b, T in enumerate(mc.sizes):
        c32, c64 = R.match_oracle(mc, b), R.match_oracle(mc, b, torch.float64)
        assert tuple(c32.shape) == (R.MATCH_Q, T) and bool(torch.isfinite(c32).all()) and bool(torch.isfinite(c64).all())
        p = mc.logits[b].sigmoid()
        assert torch.equal(R.cost_of_p(p, mc.boxes[b], mc.tgt[b]), c32)                                  # the restated class term is the oracle's
        lo, hi = R.match_bracket(mc, b)
        assert bool((lo <= c32).all()) and bool((c32 <= hi).all())
        exact = mc.logits[b, :, 0] >= R.EXACT_FROM
        assert bool((p[exact, 0] == 1.0).all()) and torch.equal(lo[exact], hi[exact])                       # zero width from logit 20 up
        assert float(np.exp(-R.EXACT_FROM)) < 2.0 ** -26
        fl = R.cost_floor(mc, b)
        print(f"COSTFLOOR {mc.name} image {b} T {T}: floor {fl:.2e}, widest bracket {float((hi - lo).max()) if T else 0.0:.2e}")
        # the cap, on the rows compared with fp64 (R.well_rows); no such claim between logits 2 and 30, the band included
        assert R.FACTOR * fl <= R.EXISTING["cost"], fl
        q, q2 = mc.dup_q                                                                                 # exact ties of the cost
        assert torch.equal(c32[q], c32[q2])
        if b in mc.dup_t:
            assert torch.equal(c32[:, mc.dup_t[b][0]], c32[:, mc.dup_t[b][1]])


def test_the_band_is_where_the_fp32_class_cost_loses_its_bits():
    """The figures of DESIGN.md: fp32 against fp64 of the reference's own expression, and what 2 ulp of p are worth."""
    x = torch.tensor([7.0, 12.0, 18.0, 14.0, 16.0])
    diff = (R.class_cost_of_p(x.sigmoid()).double() - R.class_cost_of_p(x.double().sigmoid())).abs() * 2.0
    print("BAND fp32 - fp64 of the weighted class cost at", x.tolist(), diff.tolist())
    assert 2e-5 < float(diff[0]) < 2e-3 and 7e-4 < float(diff[1]) < 7e-2 and 0.07 < float(diff[2]) < 7.0
    p = x.sigmoid()
    width = (R.class_cost_of_p(R.moved(p, x, -2)) - R.class_cost_of_p(R.moved(p, x, +2))).abs() * 2.0
    print("BAND width of +-2 ulp", width.tolist())
    assert float(width[1]) > 0.01 and float(width[3]) > 0.1 and float(width[4]) > 1.0


@pytest.mark.parametrize("launch", list(R.MATCH_LAUNCHES))
def test_pinned_duplicate_target_assignments_are_decided_by_more_than_the_bracket(launch):
    """The condition under which the GPU test may ask ops.lsap on the device cost for the CPU oracle's indices (up to duplicates): the fp32
    oracle's optimum beats the best other assignment by more than the summed bracket widths, each widened by 2e-6 (1 + |c|)."""
    mc = R.match_case(launch, "pinned")
    idx = OC.hungarian_match({"pred_logits": mc.logits, "pred_boxes": mc.boxes}, [{"boxes": t} for t in mc.tgt])
    for b, T in enumerate(mc.sizes):
        if T == 0:
            assert len(idx[b][0]) == 0
            continue
        c32 = R.match_oracle(mc, b)
        lo, hi = R.match_bracket(mc, b)
        width = (hi - lo).double() + 2 * R.EXISTING["cost"] * (1 + c32.double().abs())
        ii, jj = idx[b][0].numpy(), idx[b][1].numpy()
        gap = R.second_best_gap(c32.double().numpy(), ii, jj, mc.dup_q, mc.dup_t.get(b), oracle_lsap.linear_sum_assignment)
        m = min(R.MATCH_Q, T)
        budget = 2 * float(width.flatten().topk(m).values.sum())                                         # both assignments move by at most this
        print(f"GAP {mc.name} image {b}: second best + {gap:.3e}, summed widths {budget:.3e}")
        assert gap > budget, (b, gap, budget)
