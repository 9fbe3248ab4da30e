"""What the horizon sweeps reach (no GPU): tests/horizon_cases.py restates the launcher's arithmetic; here the sweeps'
horizons are run through it and the coverage the sweep tests claim is asserted, per model, instead of assumed."""
import pytest

import horizon_cases as HC


def test_block_shape_at_known_horizons():
    # (nblocks, nctl_last, nv_last, tail, nfull, prune)
    assert HC.block_shape("diff_drive", 50) == (7, 1, 2, False, 6, True)       # C2: H - 1 = 6 * 8 + 1
    assert HC.block_shape("diff_drive", 15) == (2, 6, 7, True, 2, False)       # the reference's default: the NCTL = 6 form
    assert HC.block_shape("full_body", 80) == (10, 7, 6, True, 10, True)       # C4: seven of the last block's eight steps
    assert HC.block_shape("full_body", 9) == (2, 0, -1, False, 1, False)       # the last block: final state only, nothing consumed
    assert HC.block_shape("diff_drive", 3) == (1, 2, 3, False, 0, False)
    assert HC.block_shape("diff_drive", 5) == (1, 4, 5, True, 1, False)        # block 0 is the partial block
    assert HC.block_shape("diff_drive", 16) == (2, 7, 8, True, 2, False)       # the last unpruned horizon
    assert HC.block_shape("diff_drive", 17) == (3, 0, 1, False, 2, True)


@pytest.mark.parametrize("sweep", ["single", "batch"])
@pytest.mark.parametrize("model", HC.MODELS)
def test_sweep_reaches_every_tail_form(model, sweep):
    hs = HC.SINGLE_H if sweep == "single" else HC.BATCH_H
    shapes = {H: HC.block_shape(model, H) for H in hs}
    # every nctl: 0 .. 7 in a last block (H - 1 = 8 m puts the m-th full batch in the block BEFORE the last, whose own nctl is
    # 0: a last block never has 8), 8 in the blocks before it
    assert {s[1] for s in shapes.values()} == set(range(0, 8))
    assert {n for H in hs for n in HC.producer_steps(H)} == set(range(0, 9))
    # every pc_consume<nv>: as the last block's for diff drive and steering; full body's last block covers at most 6 states
    # (nstates = H - 2), its widths 7 and 8 are the block before (H = 9, 17, 25: seven states in the last block consumed)
    last_nv = {s[2] for s in shapes.values() if s[2] > 0}
    assert last_nv == (set(range(1, 7)) if model == "full_body" else set(range(1, 9)))
    assert {nv for H in hs for nv in HC.consumer_widths(model, H)} == set(range(1, 9))
    assert any(HC.consumer_widths(model, H)[-1] == 7 for H in hs)
    # both sides of kPartialMin, the boundary itself included, in a last block and as the only block
    assert {HC.K_PARTIAL_MIN - 1, HC.K_PARTIAL_MIN} <= {s[1] for s in shapes.values()}
    assert {s[3] for s in shapes.values()} == {False, True}
    assert all(s[3] == (HC.K_PARTIAL_MIN <= s[1] < HC.K_TU) for s in shapes.values())
    # both sides of the pruning switch
    assert shapes[16][5] is False and shapes[17][5] is True
    # one block that is itself the partial block: the prologue's normals feed a masked batch, nfull = 1
    one = [H for H, s in shapes.items() if s[0] == 1 and s[3]]
    assert one and all(shapes[H][4] == 1 for H in one)
    assert {shapes[H][1] for H in one} == {4, 5, 6, 7}
    # every residue with one, two and three full blocks in front of it (the batch sweep starts inside the first block)
    for nblocks in (2, 3, 4):
        got = {s[1] for s in shapes.values() if s[0] == nblocks}
        assert got == (set(range(0, 8)) if nblocks < 4 else {0, 1}), (nblocks, got)
    # nfull follows the kernel's own two formulas
    for H, (nblocks, nctl, nv, tail, nfull, prune) in shapes.items():
        steps = HC.producer_steps(H)
        assert nfull == sum(1 for n in steps if n == HC.K_TU or (tail and n >= HC.K_PARTIAL_MIN)), H
        assert steps[-1] == nctl and len(steps) == nblocks


def test_batch_sweep_starts_where_full_body_has_a_state_to_cover():
    assert HC.nstates("full_body", 4) <= 2 < HC.nstates("full_body", HC.BATCH_H[0])
    assert HC.BATCH_H[-1] == HC.SINGLE_H[-1] == 26
