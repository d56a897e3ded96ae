"""The population DADDPG update (armenv_daddpg_pop_update through armenv.fused_daddpg_pop.FusedDADDPGPopulation) on cuda:0.  Its
oracle is the single-learner update: every sum of the update has one fixed order that does not depend on the grid, so member p of a
population update equals armenv_daddpg_update (armenv.fused_daddpg.FusedDADDPG) on member p's tensors BIT FOR BIT -- no tolerance
anywhere below."""
import json

import pytest
import torch

import pop_common as K

pytestmark = pytest.mark.gpu
KIND = "daddpg"


@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("B", [1, 257, 1000])
@pytest.mark.parametrize("P", [1, 2, 5])
def test_every_member_equals_the_single_update_bit_for_bit(P, B, D):
    """Four consecutive updates (total_it 6..9: actor 1, actor 2 and with it the target critic's soft update, twice) of P members
    with different random nets, moments and batches.  After every update each of member p's 72 tensors and loss[p] equals a
    FusedDADDPG that started from member p's state and was stepped by armenv_daddpg_update on member p's batch; what the update must
    not write -- the other actor, its target and moments, and with actor 1 the target critic -- is bitwise what it was."""
    gen = K.generator(1000 * P + B + D)
    pop = K.population(KIND, P, D, gen)
    singles = [pop.export_member(p) for p in range(P)]
    assert singles[0].total_it == 5 and (singles[0].actor1_step, singles[0].actor2_step, singles[0].critic_step) == (2, 3, 5)
    for it in range(4):
        k = 1 if (pop.total_it + 1) % 2 == 0 else 2
        written, untouched = K.stack_names(pop, k)
        assert sorted(written + untouched) == sorted(pop.stacks)
        before = {name: [t.clone() for t in pop.stacks[name]] for name in pop.stacks}
        batch = K.batch(gen, P, B, D)
        loss = pop.train(batch)
        assert tuple(loss.shape) == (P,)
        for p, single in enumerate(singles):
            ls = single.train(K.member_batch(batch, p))
            assert torch.equal(ls, loss[p]), (it, p, float(ls), float(loss[p]))
            bad = [i for i, (x, y) in enumerate(zip(K.state(pop, p), pop._single_state(single))) if not torch.equal(x, y)]
            assert not bad, (it, p, bad)
        for name in untouched:
            assert all(torch.equal(x, y) for x, y in zip(before[name], pop.stacks[name])), (it, name)
        for name in written:
            assert not any(torch.equal(x, y) for x, y in zip(before[name], pop.stacks[name])), (it, name)
    assert (pop.total_it, pop.critic_step, pop.actor1_step, pop.actor2_step) == (9, 9, 4, 5)
    assert all(bool(torch.isfinite(t).all()) for six in pop.stacks.values() for t in six)
    if P > 1:
        assert not torch.equal(pop.stacks["actor1"][0][0], pop.stacks["actor1"][0][1])
        assert not torch.equal(loss[0], loss[1])


def test_members_do_not_leak_into_each_other():
    K.check_members_do_not_leak(KIND)


def test_nothing_is_written_outside_the_stacks_and_the_workspace():
    K.check_canaries(KIND)


def test_one_member_equals_the_single_update_on_the_same_tensors():
    K.check_one_member_equals_the_single_update_on_the_same_tensors(KIND)


def test_population_update_is_deterministic_across_runs_and_streams():
    K.check_determinism(KIND)


def test_population_update_captured_in_a_graph_equals_direct_calls():
    K.check_graph_capture(KIND)


def test_zero_learning_rates_and_tau_leave_every_member_unchanged():
    K.check_zero_learning_rates(KIND)


def test_load_and_export_member_round_trip():
    K.check_round_trip(KIND)


def test_population_training_loop_learns_reach_for_every_member():
    """train_reach_population(members=2, algo="daddpg") at the size, iteration count and bar of
    test_training_loop_learns_reach_with_the_fused_daddpg_learner (each member is that run with its own seed): >= 90 % success over
    the last log window and more than 5000 episodes for every member; the members' curves are not identical, their seeds being
    independent."""
    from armenv.fused_daddpg_pop import FusedDADDPGPopulation
    from armenv.train_pop import train_reach_population
    hist = []
    pop, _ = train_reach_population(members=2, num_envs=1024, iterations=140, updates=48, batch_size=2048, log_every=20,
                                    log=lambda s_: hist.append(json.loads(s_)), algo="daddpg")
    assert isinstance(pop, FusedDADDPGPopulation) and pop.total_it > 0 and len(hist) == 7
    rates = hist[-1]["success_rate"]
    print("success rates per log window:", [[round(r, 3) for r in h["success_rate"]] for h in hist])
    assert len(rates) == 2 and min(rates) >= 0.9, [[round(r, 2) for r in h["success_rate"]] for h in hist]
    assert min(hist[-1]["episodes"]) > 5000
    assert [h["success_rate"][0] for h in hist] != [h["success_rate"][1] for h in hist]


def test_the_default_population_is_still_td3():
    """train_reach_population() with its defaults (here: a handful of tiny iterations) returns a FusedTD3Population."""
    from armenv.fused_td3_pop import FusedTD3Population
    from armenv.train_pop import train_reach_population
    pop, hist = train_reach_population(members=2, num_envs=64, iterations=4, rollout_steps=16, updates=2, batch_size=64,
                                       window_steps=64, max_steps=20, log_every=2, log=lambda s_: None)
    assert type(pop) is FusedTD3Population and len(hist) == 2 and pop.total_it > 0
