"""The population DATD3 / DARC update (armenv_datd3_pop_update through armenv.fused_datd3_pop.FusedDATD3Population and
FusedDARCPopulation) on cuda:0.  Its oracle is the single-learner update: every sum of the update has one fixed order that does not
depend on the grid, so member p of a population update equals armenv_datd3_update (armenv.fused_datd3.FusedDATD3 / FusedDARC, seed
``seed + p``) on member p's tensors BIT FOR BIT -- no tolerance anywhere below."""
import pytest
import torch

import pop_common as K

pytestmark = pytest.mark.gpu
KINDS = ("datd3", "darc")


@pytest.mark.parametrize("given_noise", [True, False], ids=["noise_given", "noise_in_kernel"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [6, 9])
@pytest.mark.parametrize("B", [1, 257, 1000])
@pytest.mark.parametrize("P", [1, 2, 5])
def test_every_member_equals_the_single_update_bit_for_bit(P, B, D, kind, given_noise):
    """Two `train` calls (updates 7..10: k = 1, 2, 1, 2) of P members with different random nets, moments and batches, stepped
    update by update.  After every update each of member p's 96 tensors and loss[p] equals a single learner that started from
    member p's state, has seed + p, and was stepped by armenv_datd3_update on member p's batch (and member p's noise, when given);
    actor / critic `other`, their targets and their moments are bitwise what they were."""
    gen = K.generator(1000 * P + B + D)
    pop = K.population(kind, P, D, gen)
    singles = [pop.export_member(p) for p in range(P)]
    assert [s.seed for s in singles] == [11 + p for p in range(P)] and singles[0].total_it == 6 and singles[0].critic2_step == 3
    for it in range(2):
        batch = K.batch(gen, P, B, D)
        for k in (1, 2):                                   # what train(batch, noise) does, looked at after each of its updates
            written, untouched = K.stack_names(pop, k)
            assert sorted(written + untouched) == sorted(pop.stacks)
            before = {name: [t.clone() for t in pop.stacks[name]] for name in pop.stacks}
            noise = K.noise_for(gen, P, B) if given_noise else None
            loss = pop.update(batch, update_a1=(k == 1), noise=noise)
            assert tuple(loss.shape) == (P,)
            for p, single in enumerate(singles):
                ls = single.update(K.member_batch(batch, p), update_a1=(k == 1), noise=None if noise is None else noise[p])
                assert torch.equal(ls, loss[p]), (it, k, p, float(ls), float(loss[p]))
                bad = [i for i, (x, y) in enumerate(zip(K.state(pop, p), pop._single_state(single))) if not torch.equal(x, y)]
                assert not bad, (it, k, p, bad)
            for name in untouched:
                assert all(torch.equal(x, y) for x, y in zip(before[name], pop.stacks[name])), (it, k, name)
            for name in written:
                assert not any(torch.equal(x, y) for x, y in zip(before[name], pop.stacks[name])), (it, k, name)
    assert pop.total_it == 10 and (pop.actor1_step, pop.critic1_step, pop.actor2_step, pop.critic2_step) == (5, 5, 5, 5)
    assert all(bool(torch.isfinite(t).all()) for six in pop.stacks.values() for t in six)
    if P > 1:
        assert not torch.equal(pop.stacks["actor1"][0][0], pop.stacks["actor1"][0][1])
        assert not torch.equal(loss[0], loss[1])


@pytest.mark.parametrize("given_noise", [True, False], ids=["noise_given", "noise_in_kernel"])
@pytest.mark.parametrize("kind", KINDS)
def test_train_is_update_one_then_update_two_with_consecutive_draws(kind, given_noise):
    """Two population `train` calls against the single learners' `train` on the members' slices: both losses of every call and the
    whole state afterwards, bit for bit; total_it counts updates."""
    P, B, D = 3, 257, 6
    gen = K.generator(17)
    pop = K.population(kind, P, D, gen)
    singles = [pop.export_member(p) for p in range(P)]
    for it in range(2):
        batch = K.batch(gen, P, B, D)
        noise = (K.noise_for(gen, P, B), K.noise_for(gen, P, B)) if given_noise else None
        l1, l2 = pop.train(batch, noise=noise)
        assert pop.total_it == 6 + 2 * (it + 1)
        for p, single in enumerate(singles):
            s1, s2 = single.train(K.member_batch(batch, p), noise=None if noise is None else (noise[0][p], noise[1][p]))
            assert torch.equal(s1, l1[p]) and torch.equal(s2, l2[p]), (it, p)
            assert all(torch.equal(x, y) for x, y in zip(K.state(pop, p), pop._single_state(single))), (it, p)
    if not given_noise:                                    # members draw different noise: seed + p
        a, b = K.population(kind, 2, D, None, seed=11), K.population(kind, 2, D, None, seed=12)
        b.load_member(0, a.export_member(1))
        shared = K.batch(gen, 1, B, D)
        two = {k: torch.cat([v, v]) for k, v in shared.items()}
        la, lb = a.update(two), b.update(two)
        assert torch.equal(la[1], lb[0])                   # member 1 of seed 11 is member 0 of seed 12: key seed + p


@pytest.mark.parametrize("kind", KINDS)
def test_members_do_not_leak_into_each_other(kind):
    K.check_members_do_not_leak(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_is_written_outside_the_stacks_and_the_workspace(kind):
    K.check_canaries(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_one_member_equals_the_single_update_on_the_same_tensors(kind):
    K.check_one_member_equals_the_single_update_on_the_same_tensors(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_population_update_is_deterministic_across_runs_and_streams(kind):
    K.check_determinism(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_population_update_captured_in_a_graph_equals_direct_calls(kind):
    K.check_graph_capture(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_zero_learning_rates_and_tau_leave_every_member_unchanged(kind):
    K.check_zero_learning_rates(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_load_and_export_member_round_trip(kind):
    K.check_round_trip(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_population_training_loop_runs_two_updates_per_loop_update(kind):
    """A dozen small iterations of train_reach_population: total_it advances by two per loop update (one `train`), and every
    member's parameters stay finite."""
    from armenv.train_pop import train_reach_population
    counted = []
    pop, hist = train_reach_population(members=2, num_envs=64, iterations=12, rollout_steps=16, updates=3, batch_size=64,
                                       window_steps=64, max_steps=20, log_every=4, log=counted.append, algo=kind)
    assert type(pop) is K.classes(kind)[0] and len(hist) == 3 and len(counted) == 3
    assert pop.total_it > 0 and pop.total_it % (2 * 3) == 0                # whole iterations of 3 loop updates, 2 updates each
    assert pop.actor1_step == pop.critic1_step == pop.actor2_step == pop.critic2_step == pop.total_it // 2
    assert all(bool(torch.isfinite(t).all()) for six in pop.stacks.values() for t in six)
    assert all(0.0 <= r <= 1.0 for h in hist for r in h["success_rate"])
