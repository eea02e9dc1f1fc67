"""The lives and walks of tests/context_life.py, checked without a GPU: they are deterministic, between them they use every step kind
and name every group of context state that outlives a call, and no two consecutive calls of a life draw their inputs from one seed."""
import context_life as CL

# the members of emi_ctx_s (etol_amd/csrc/emi_ctx.hpp) that carry state from call to call, by group; written here, not read from
# context_life: a group nobody is after fails this test
STATE_GROUPS = {
    "operator copies": ("d_D", "d_De", "d_Do", "d_Dfrag", "has_dfrag"),
    "work tables": ("pass_work",),
    "slab, tickets, cost partials": ("d_slab", "d_tile_ticket", "d_ticket", "d_cost_part"),
    "keep record": ("keep",),
    "dirty flags": ("adj_dirty", "ode_dirty", "delay_dirty", "adjw_dirty", "odel_dirty"),
    "delay operators": ("d_W", "d_uext"),
    "block-term and interior-point lists": ("blk_key", "ipm_key"),
    "model program": ("rtc", "pvars", "path_has_track"),
    "host-form staging": ("s_X", "s_VALS", "host_stage"),
    "Newton-step workspaces": ("kkt", "kkt_shard"),
    "driver workspaces": ("ipm_solve", "ipm_ladder", "start_guess"),
}


def everything():
    return {**{name: make() for name, make in CL.LIVES.items()}, **{f"walk{seed}": CL.seeded_walk(seed) for seed in (1, 2, 3)}}


def test_lives_and_walks_are_deterministic():
    assert everything() == everything()
    assert all(len(CL.seeded_walk(seed)) == 34 for seed in (1, 2, 3))            # four steps of set-up, then thirty
    assert CL.seeded_walk(1) != CL.seeded_walk(2) != CL.seeded_walk(3)


def test_every_step_kind_occurs_in_some_life():
    used = set()
    for steps in (make() for make in CL.LIVES.values()):
        used |= {st.kind for st in steps if st.kind in CL.SETTERS} | {kind for kind, _ in CL.calling_steps(steps)}
    assert used == set(CL.SETTERS) | set(CL.CALLS), used ^ (set(CL.SETTERS) | set(CL.CALLS))


def test_every_group_of_context_state_is_some_lifes_target():
    assert set(CL.TARGETS) == set(CL.LIVES)
    named = {m for members in CL.TARGETS.values() for m in members}
    header = open(CL.ROOT + "/etol_amd/csrc/emi_ctx.hpp").read()
    for group, members in STATE_GROUPS.items():
        for m in members:
            assert m in header, f"{m} is no member of emi_ctx_s any more"
            assert m in named, f"no life is after {m} ({group})"


def test_no_two_consecutive_calls_share_a_seed():
    for name, steps in everything().items():
        calls = CL.calling_steps(steps)
        seeds = [seed for _, seed in calls]
        assert all(s >= 0 for s in seeds), name
        assert len(set(seeds)) == len(seeds), name      # (none repeats at all)
        assert all(a != b for a, b in zip(seeds, seeds[1:])), name


def test_walks_stay_in_the_cheap_part_of_the_alphabet():
    for seed in (1, 2, 3):
        for st in CL.seeded_walk(seed):
            assert st.kind in CL.SETTERS or st.kind in CL.WALK_CALLS
            assert st.arg("source") is None
            if st.kind == "mesh":
                assert st.arg("M") in (33, 65, 128, 256)
            if st.kind == "batch":
                assert st.arg("B") <= 80


def test_the_fork_condition_of_the_adjoint_is_the_librarys():
    """context_life.adjoint_forks, by which the stream-order test chooses the shape of its "second stream" cases, restates one line of
    emi_adjoint.hip: that line and its constant are still there, and the shapes still lie on either side of it"""
    import re
    src = open(CL.ROOT + "/etol_amd/csrc/emi_adjoint.hip").read()
    cus = int(re.search(r"constexpr int ADJ_CUS = (\d+);", src).group(1))
    assert "bool adjoint_side_by_side(int B, int ns, int M) { return ((B * ns + 95) / 96) * ((M + 127) / 128) >= ADJ_CUS; }" in src
    assert CL.adjoint_forks(2048, 6, 256, cus) and not CL.adjoint_forks(17, 6, 128, cus)
    assert CL.adjoint_forks.__defaults__ == (cus,)
