"""The population TD3 update (armenv_td3_pop_update through armenv.fused_td3_pop.FusedTD3Population) on cuda:0.  Its oracle is the
single-learner update: every sum of the update has one fixed order that does not depend on the grid, so member p of a population
update equals armenv_td3_update (armenv.fused_td3.FusedTD3) on member p's tensors BIT FOR BIT -- no tolerance anywhere below."""
import json

import pytest
import torch

import pop_common as K

pytestmark = pytest.mark.gpu
KIND = "td3"


@pytest.mark.parametrize("given_noise", [True, False], ids=["noise_given", "noise_in_kernel"])
@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("B", [1, 64, 257, 1000])
@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_every_member_equals_the_single_update_bit_for_bit(P, B, D, given_noise):
    """Six consecutive updates (total_it 5..10: two with the actor step) of P members with different random nets, moments and
    batches.  After every update each of member p's 72 tensors and loss[p] equals a FusedTD3 that started from member p's state,
    has seed + p, and was stepped by armenv_td3_update on member p's batch (and member p's noise, when given); without the actor
    step the actor, its moments and the three targets are bitwise what they were."""
    gen = K.generator(1000 * P + B + D)
    pop = K.population(KIND, P, D, gen)
    singles = [pop.export_member(p) for p in range(P)]
    assert [s.seed for s in singles] == [11 + p for p in range(P)] and singles[0].total_it == 4
    actor_steps = 0
    for it in range(6):
        with_actor = (pop.total_it + 1) % pop.policy_freq == 0
        written, untouched = K.stack_names(pop, with_actor)
        assert sorted(written + untouched) == sorted(pop.stacks)
        before = {name: [t.clone() for t in pop.stacks[name]] for name in pop.stacks}
        batch = K.batch(gen, P, B, D)
        noise = K.noise_for(gen, P, B) if given_noise else None
        loss = pop.train(batch, noise=noise)
        assert tuple(loss.shape) == (P,)
        actor_steps += with_actor
        for p, single in enumerate(singles):
            ls = single.train(K.member_batch(batch, p), noise=None if noise is None else noise[p])
            assert torch.equal(ls, loss[p]), (it, p, float(ls), float(loss[p]))
            bad = [k for k, (x, y) in enumerate(zip(K.state(pop, p), pop._single_state(single))) if not torch.equal(x, y)]
            assert not bad, (it, p, bad)
        for name in untouched:
            assert all(torch.equal(x, y) for x, y in zip(before[name], pop.stacks[name])), (it, name)
        for name in written:
            assert not any(torch.equal(x, y) for x, y in zip(before[name], pop.stacks[name])), (it, name)
    assert actor_steps == 2 and pop.actor_step == 3 and pop.critic_step == 10
    assert all(bool(torch.isfinite(t).all()) for six in pop.stacks.values() for t in six)
    if P > 1:
        assert not torch.equal(pop.stacks["actor"][0][0], pop.stacks["actor"][0][1])


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
    """train_reach_population(members=3) at the size, iteration count and bar of test_training_loop_learns_reach_with_the_fused_learner
    (each member is that run with its own seed): >= 90 % success over the last log window for every member; the members' curves
    are not identical, their seeds being independent."""
    from armenv.fused_td3_pop import FusedTD3Population
    from armenv.train_pop import train_reach_population
    hist = []
    pop, _ = train_reach_population(members=3, num_envs=1024, iterations=140, updates=48, batch_size=2048, log_every=20,
                                    log=lambda s_: hist.append(json.loads(s_)))
    assert isinstance(pop, FusedTD3Population) and pop.total_it > 0 and len(hist) == 7
    rates = hist[-1]["success_rate"]
    print("success rates per log window:", [[round(r, 3) for r in h["success_rate"]] for h in hist])
    assert len(rates) == 3 and min(rates) >= 0.9, [[round(r, 2) for r in h["success_rate"]] for h in hist]
    assert min(hist[-1]["episodes"]) > 5000
    curves = [[h["success_rate"][p] for h in hist] for p in range(3)]
    assert curves[0] != curves[1] and curves[1] != curves[2] and curves[0] != curves[2]
