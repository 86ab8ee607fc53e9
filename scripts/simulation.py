#!/usr/bin/env python3
"""Counterpart of the reference's scripts/simulation.py (load tables, run greedy landing episodes): evaluates a
pair of Q tables in the vectorised simulator and reports how the episodes end.

    python scripts/simulation.py [--tables DIR] [--envs 4096] [--level 4] [--flavour simulation|training] [--mode paper|reference]
                                 [--rollout] [--report] [--trace-out FILE.npz [--trace-envs 8]] [--map-out FILE.npz [--map-episodes 1]]
                                 [--model-out FILE.npz [--model-eps 0.1]] [--grid-out FILE.npz --grid FIELD=v1,v2,... [--grid ...]]
                                 [--returns-out FILE.npz [--returns-eps 0.1] [--returns-gamma 0.99]]
                                 [--split-out FILE.npz --split-by NAME[,NAME...]|all [--split-eps 0.1] [--split-seeds 1]]
                                 [--cut-out FILE.npy --cut-by FEATURE [--cut-eps 0.1]]
Default tables: tests/golden/assets (a data copy of the reference's stage-4 policy).
--rollout flies all first episodes in one launch (dql_rollout) instead of one launch per agent period; --report prints what the episodes looked like at
their end (the counterpart of the `info` dictionary the reference prints per episode, scripts/simulation.py:52-56) and --trace-out saves the per-period
flight record of the first envs; both imply --rollout.
--map-out writes where the tables' greedy policy flies (dql_score_map): `visits` [2835], the decisions counted by cell, and
`last_cell_by_code` [codes, 2835], the histogram of the x cell of each finished episode's last decision by terminal code, with `by_code` and `columns`.
--model-out writes the empirical transition model of the discretised MDP under the tables' eps-greedy policy (dql_model): `pairs`
[2835, 945], `reward_fx` [2835], `terminal` [2835, codes] and `visits` [2835], with `by_code`, `columns`, `steps_sum` and `eps` (--model-eps; --map-episodes
episodes per env).
--returns-out writes the realised discounted returns of the tables' eps-greedy policy per (state, action) cell and what they say about the tables' values
(dql_returns): `visits` [2835] and `return_fx` [2835] (the returns-to-go of the finished episodes' decisions, summed, in units of 2^-26),
`cut_decisions`, `by_code`, `columns`, `steps_sum`, `eps`, `gamma`, and `evaluation.value_calibration`'s per-cell arrays `mean_return`, `bias_a`, `bias_b`,
`bias_mean` (Q minus mean return; NaN below 30 visits); the report carries its summary (--map-episodes episodes per env).
--split-out asks which variable is hidden state of the 945 states (dql_model_split): per --split-by feature (names of ops.SPLIT_FEATURES,
e.g. pitch_sp,mp_phase,prev_action, or `all`) three passes over identical flights — cut = +inf for the feature's per-state means, the split at the means, and one
coin pass for the sampling floor (--split-seeds seeds summed, --map-episodes episodes per env).  The file holds per feature `pairs_NAME` [2, 2835, 945],
`terminal_NAME`, `reward_fx_NAME`, `feat_sum_fx_NAME` [945] and `cut_NAME` [945], and the coin's; `evaluation.aliasing_table`'s rows are printed and reported.
--cut-out writes the cut a refined ensemble is trained with (scripts/ensemble_training.py --refine FEATURE --refine-cut FILE.npy): the tables
are flown at each of the levels 0 .. 4 in the training flavour with one dql_model_split pass per level (cut = +inf, --cut-eps, --map-episodes episodes per env), and
`evaluation.refinement_cut` merges the per-state means of --cut-by into one float64 [945] array; a state that is unvisited at its own level stays at +inf.
--grid-out scores the tables over the Cartesian product of the --grid axes in ONE launch (dql_score_grid): `--grid mp_t_x=0.8,1.2,1.6 --grid
trajectory=0,1` flies six scenarios that differ from the flavour's config in those fields only (the first axis varies slowest).  The file holds `by_code`
[S, codes + 1], `steps_sum` [S], `touch_hist` [S, 8] (touchdowns by their offset from the platform centre), `touch_edges` [S, 7], `columns`, one array per
axis with its value per scenario, and `evaluation.robustness_table`'s columns; the report names the worst scenario (--map-episodes episodes per env).
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def evaluate(tables_dir, n_envs=4096, level=4, max_steps=600, seed=123, dtype=None, flavour="simulation", device=0, method="stepwise", **cfg_kw):
    """Greedy roll-outs of the tables saved in `tables_dir`; returns the terminal histogram of the FIRST episode of every env."""
    from dql_multirotor_landing_amd.double_q_learning import DoubleQLearningAgent
    from dql_multirotor_landing_amd.evaluation import first_episode_outcomes
    agent = DoubleQLearningAgent.load(Path(tables_dir))
    return first_episode_outcomes(agent._padded(), n_envs, level, max_steps, seed, dtype, flavour, device, method=method, **cfg_kw)


def evaluate_records(tables_dir, n_envs=4096, level=4, max_steps=600, seed=123, dtype=None, flavour="simulation", device=0, trace_envs=0, **cfg_kw):
    """The per-episode records (and the trace of the first `trace_envs` envs) of the same roll-outs, from the one-launch operator."""
    from dql_multirotor_landing_amd.double_q_learning import DoubleQLearningAgent
    from dql_multirotor_landing_amd.evaluation import rollout_records
    agent = DoubleQLearningAgent.load(Path(tables_dir))
    return rollout_records([agent._padded()], n_envs, level, max_steps, seed, dtype, flavour, device, trace_envs=trace_envs, **cfg_kw)


def evaluate_map(tables_dir, n_envs=4096, level=4, max_steps=600, seed=123, dtype=None, flavour="simulation", device=0, episodes=1, **cfg_kw):
    """The map of the same greedy flights and the last-cell histogram by terminal code, from one launch of the mapping scorer."""
    import numpy as np
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.config import CHECK_NAMES
    from dql_multirotor_landing_amd.double_q_learning import DoubleQLearningAgent
    qa, qb, _ = DoubleQLearningAgent.load(Path(tables_dir))._padded()
    cfg = evaluation._flavour_config(flavour, level, dtype, cfg_kw)
    r = ops.score_map(cfg, qa, qb, n_envs, seed, episodes=episodes, max_steps=max_steps, log=True, device=device)
    by_code = np.stack([evaluation.failure_origins(r["ep_code"], r["ep_last_cell"], [k], 1)[0] for k in range(len(CHECK_NAMES))])
    return {"visits": r["visits"][0], "last_cell_by_code": by_code, "by_code": r["by_code"][0], "columns": np.array(r["columns"]), "steps_sum": r["steps_sum"][0]}


def evaluate_model(tables_dir, n_envs=4096, level=4, max_steps=600, seed=123, dtype=None, flavour="simulation", device=0, episodes=1, eps=0.1, **cfg_kw):
    """The empirical transition model of the same flights under the tables' eps-greedy policy, from one launch of the model operator."""
    import numpy as np
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.double_q_learning import DoubleQLearningAgent
    qa, qb, _ = DoubleQLearningAgent.load(Path(tables_dir))._padded()
    cfg = evaluation._flavour_config(flavour, level, dtype, cfg_kw)
    r = ops.transition_model(cfg, qa, qb, n_envs, seed, eps, episodes=episodes, max_steps=max_steps, device=device)
    out = {f: r[f][0] for f in ("pairs", "reward_fx", "terminal", "visits", "by_code", "steps_sum")}
    out.update({"columns": np.array(r["columns"]), "eps": np.float64(eps)})
    return out


def evaluate_split(tables_dir, features, n_envs=4096, level=4, max_steps=600, seed=123, dtype=None, flavour="simulation", device=0, episodes=1, eps=0.1, n_seeds=1, min_visits=30,
                   **cfg_kw):
    """Which variable is hidden state of the 945 states: per named feature the transition model split at the feature's per-state mean, over identical flights
    (seeds seed .. seed + n_seeds - 1, summed): pass 1 with cut = +inf gives the means, pass 2 splits at them, one coin pass gives the sampling floor.  Returns
    (arrays for the .npz, evaluation.aliasing_table's rows; with two or more seeds also the row of the odd seeds' coin against the even seeds' coin)."""
    import numpy as np
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.double_q_learning import DoubleQLearningAgent
    qa, qb, _ = DoubleQLearningAgent.load(Path(tables_dir))._padded()
    cfg = evaluation._flavour_config(flavour, level, dtype, cfg_kw)
    summed = ("pairs", "reward_fx", "terminal", "feat_sum_fx", "by_code", "steps_sum")

    def fly(feature, cut, seeds):
        total = None
        for s in seeds:
            r = ops.split_model(cfg, qa, qb, n_envs, s, eps, feature, cut, episodes=episodes, max_steps=max_steps, device=device)
            total = {f: r[f].copy() for f in summed} if total is None else {f: total[f] + r[f] for f in summed}
        return total

    seeds = [seed + k for k in range(n_seeds)]
    by_feature, out = {}, {"eps": np.float64(eps), "seeds": np.array(seeds), "features": np.array(list(features))}
    for name in features:
        cut = evaluation.feature_means(fly(name, np.inf, seeds))[0]
        by_feature[name] = fly(name, cut, seeds)
        out[f"cut_{name}"] = cut
        out.update({f"{f}_{name}": by_feature[name][f][0] for f in ("pairs", "reward_fx", "terminal", "feat_sum_fx")})
    coins = [fly("coin", 0.5, seeds[k::2]) for k in range(min(2, n_seeds))]
    coin = coins[0] if len(coins) == 1 else {f: coins[0][f] + coins[1][f] for f in summed}
    out.update({f"{f}_coin": coin[f][0] for f in ("pairs", "reward_fx", "terminal")})
    out.update({"by_code": coin["by_code"][0], "steps_sum": coin["steps_sum"][0]})
    table = evaluation.aliasing_table(by_feature, coin, min_visits)
    if len(coins) == 2:
        table["coin (odd seeds)"] = evaluation.aliasing_table({"coin": coins[1]}, coins[0], min_visits)["coin"]
    return out, table


def evaluate_cut(tables_dir, feature, n_envs=4096, max_steps=600, seed=123, dtype=None, flavour="training", device=0, episodes=1, eps=0.1, **cfg_kw):
    """The cut of a refinement by `feature`: one split-model pass per level 0 .. 4 (cut = +inf) over the tables' eps-greedy flights, merged by
    `evaluation.refinement_cut`; returns (cut float64 [945], states visited per level)."""
    import numpy as np
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.double_q_learning import DoubleQLearningAgent
    qa, qb, _ = DoubleQLearningAgent.load(Path(tables_dir))._padded()
    results = [ops.split_model(evaluation._flavour_config(flavour, level, dtype, cfg_kw), qa, qb, n_envs, seed, eps, feature, np.inf, episodes=episodes, max_steps=max_steps,
                               device=device) for level in range(5)]
    cut = evaluation.refinement_cut(results)
    return cut, [int(np.isfinite(cut[189 * k:189 * (k + 1)]).sum()) for k in range(5)]


def evaluate_returns(tables_dir, n_envs=4096, level=4, max_steps=600, seed=123, dtype=None, flavour="simulation", device=0, episodes=1, eps=0.1, gamma=0.99, **cfg_kw):
    """The realised returns of the same flights under the tables' eps-greedy policy and the calibration of the tables against them; returns (arrays, summary)."""
    import numpy as np
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.double_q_learning import DoubleQLearningAgent
    qa, qb, _ = DoubleQLearningAgent.load(Path(tables_dir))._padded()
    cfg = evaluation._flavour_config(flavour, level, dtype, cfg_kw)
    r = ops.returns_map(cfg, qa, qb, n_envs, seed, eps, gamma, episodes=episodes, max_steps=max_steps, device=device)
    cal = evaluation.value_calibration(qa, qb, r["visits"][0], r["return_fx"][0], greedy=evaluation.greedy_actions(qa, qb)[0])
    out = {f: r[f][0] for f in ("visits", "return_fx", "cut_decisions", "by_code", "steps_sum")}
    out.update({"columns": np.array(r["columns"]), "eps": np.float64(eps), "gamma": np.float64(gamma)})
    out.update({f: cal[f] for f in ("mean_return", "bias_a", "bias_b", "bias_mean")})
    return out, cal["summary"]


def evaluate_grid(tables_dir, axes, n_envs=4096, level=4, max_steps=600, seed=123, dtype=None, flavour="simulation", device=0, episodes=1, **cfg_kw):
    """The same tables scored under every scenario of the grid `axes` ({field: [values]}) in one launch; returns (arrays for the .npz, labels, table)."""
    import numpy as np
    from dql_multirotor_landing_amd import evaluation, ops
    from dql_multirotor_landing_amd.config import scenario_grid
    from dql_multirotor_landing_amd.double_q_learning import DoubleQLearningAgent
    qa, qb, _ = DoubleQLearningAgent.load(Path(tables_dir))._padded()
    cfgs, labels = scenario_grid(evaluation._flavour_config(flavour, level, dtype, cfg_kw), **axes)
    r = ops.score_grid(cfgs, qa, qb, n_envs, seed, episodes=episodes, max_steps=max_steps, device=device)
    t = evaluation.robustness_table(r, labels)
    out = {"by_code": r["by_code"][:, 0], "steps_sum": r["steps_sum"][:, 0], "touch_hist": r["touch_hist"][:, 0], "touch_edges": r["touch_edges"], "columns": np.array(r["columns"])}
    out.update({f"axis_{f}": np.array([lab[f] for lab in labels]) for f in axes})
    out.update({f: t[f][:, 0] for f in ("rate", "mean_steps", "unfinished", "touch_centre", "touch_outside")})
    return out, labels, t


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", default=str(Path(__file__).resolve().parent.parent / "tests" / "golden" / "assets"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--flavour", default="simulation", choices=["simulation", "training"])
    ap.add_argument("--mode", default="paper", choices=["paper", "reference"],
                    help="observation / MDP quirk set of the roll-outs: 'paper' (default; what scripts/training.py --mode paper trains under) or the "
                         "reference's code as it is (frozen acceleration reference B19, sticky checks B8, ...: DESIGN.md section 3)")
    ap.add_argument("--rollout", action="store_true", help="fly all first episodes in one launch (dql_rollout) instead of one launch per agent period")
    ap.add_argument("--report", action="store_true", help="print episode_report: length, return and touchdown quantiles of the first episodes (implies --rollout)")
    ap.add_argument("--trace-out", default=None, metavar="FILE.npz", help="save the per-period trace of the first --trace-envs envs with its field names (implies --rollout)")
    ap.add_argument("--trace-envs", type=int, default=8)
    ap.add_argument("--map-out", default=None, metavar="FILE.npz", help="save the map of the greedy flights and the last-cell histogram by terminal code (dql_score_map)")
    ap.add_argument("--map-episodes", type=int, default=1, help="episodes per env of the --map-out launch")
    ap.add_argument("--model-out", default=None, metavar="FILE.npz", help="save the empirical transition model of the tables' eps-greedy policy (dql_model)")
    ap.add_argument("--model-eps", type=float, default=0.1, help="exploration rate of the --model-out launch, in [0, 1]")
    ap.add_argument("--returns-out", default=None, metavar="FILE.npz", help="save the realised returns per cell of the tables' eps-greedy policy and the tables' calibration (dql_returns)")
    ap.add_argument("--returns-eps", type=float, default=0.1, help="exploration rate of the --returns-out launch, in [0, 1]")
    ap.add_argument("--returns-gamma", type=float, default=0.99, help="discount of the --returns-out returns, in [0, 1]")
    ap.add_argument("--split-out", default=None, metavar="FILE.npz", help="save the transition model split by each --split-by feature at its per-state mean, and print the aliasing table (dql_model_split)")
    ap.add_argument("--split-by", default=None, metavar="NAME[,NAME...]", help="the hidden variables to split by: names of ops.SPLIT_FEATURES, or `all`")
    ap.add_argument("--split-eps", type=float, default=0.1, help="exploration rate of the --split-out launches, in [0, 1]")
    ap.add_argument("--split-seeds", type=int, default=1, help="how many seeds' flights are summed per pass (123, 124, ...)")
    ap.add_argument("--grid-out", default=None, metavar="FILE.npz", help="save the tables' score over the grid of --grid scenarios, flown in one launch (dql_score_grid)")
    ap.add_argument("--grid", action="append", default=[], metavar="FIELD=v1,v2,...", help="one axis of the --grid-out scenarios: a DqlConfig field and its values (repeatable)")
    ap.add_argument("--cut-out", default=None, metavar="FILE.npy", help="save the per-state means of --cut-by over the tables' flights at levels 0 .. 4: the cut of a refined ensemble (dql_model_split)")
    ap.add_argument("--cut-by", default=None, metavar="FEATURE", help="the hidden variable of --cut-out: a name of ops.SPLIT_FEATURES")
    ap.add_argument("--cut-eps", type=float, default=0.1, help="exploration rate of the --cut-out launches, in [0, 1]")
    a = ap.parse_args()
    if bool(a.cut_out) != bool(a.cut_by):
        ap.error("--cut-out FILE.npy and --cut-by FEATURE belong together")
    if bool(a.split_out) != bool(a.split_by):
        ap.error("--split-out FILE.npz and --split-by NAME[,NAME...] belong together")
    if bool(a.grid_out) != bool(a.grid):
        ap.error("--grid-out FILE.npz and at least one --grid FIELD=v1,v2,... belong together")
    import __graft_entry__ as g
    g.build_hip()
    from dql_multirotor_landing_amd.config import Q_PAPER, Q_REFERENCE
    quirks = Q_PAPER if a.mode == "paper" else Q_REFERENCE
    n = a.envs
    out = {"tables": a.tables, "envs": n, "level": a.level, "flavour": a.flavour, "mode": a.mode}
    if a.report or a.trace_out:
        import numpy as np
        from dql_multirotor_landing_amd.evaluation import episode_report
        rec = evaluate_records(a.tables, n, a.level, flavour=a.flavour, trace_envs=a.trace_envs if a.trace_out else 0, quirks=quirks)
        rep = episode_report(rec)[0]
        h = rep["histogram"]
        out["method"] = "rollout"
        if a.report:
            out["episode_report"] = rep
        if a.trace_out:
            np.savez(a.trace_out, trace=rec["trace"], fields=np.array(rec["trace_fields"]), code=rec["code"][0, :a.trace_envs], steps=rec["steps"][0, :a.trace_envs])
            out["trace"] = {"file": a.trace_out, "envs": a.trace_envs, "shape": list(rec["trace"].shape)}
    else:
        h = evaluate(a.tables, n, a.level, flavour=a.flavour, method="rollout" if a.rollout else "stepwise", quirks=quirks)
        out["method"] = "rollout" if a.rollout else "stepwise"
    if a.map_out:
        import numpy as np
        m = evaluate_map(a.tables, n, a.level, flavour=a.flavour, episodes=a.map_episodes, quirks=quirks)
        np.savez_compressed(a.map_out, **m)
        out["map"] = {"file": a.map_out, "episodes_per_env": a.map_episodes, "decisions": int(m["visits"].sum()), "cells_visited": int((m["visits"] > 0).sum()),
                      "busiest_cell": int(m["visits"].argmax()), "busiest_cell_visits": int(m["visits"].max())}
    if a.model_out:
        import numpy as np
        m = evaluate_model(a.tables, n, a.level, flavour=a.flavour, episodes=a.map_episodes, eps=a.model_eps, quirks=quirks)
        np.savez_compressed(a.model_out, **m)
        out["model"] = {"file": a.model_out, "eps": a.model_eps, "episodes_per_env": a.map_episodes, "decisions": int(m["visits"].sum()), "cells_visited": int((m["visits"] > 0).sum()),
                        "distinct_pairs": int((m["pairs"] > 0).sum()), "terminal_decisions": int(m["terminal"].sum())}
    if a.returns_out:
        import numpy as np
        m, summary = evaluate_returns(a.tables, n, a.level, flavour=a.flavour, episodes=a.map_episodes, eps=a.returns_eps, gamma=a.returns_gamma, quirks=quirks)
        np.savez_compressed(a.returns_out, **m)
        as_json = lambda v: {k: as_json(x) for k, x in v.items()} if isinstance(v, dict) else ([round(float(x), 4) for x in v] if isinstance(v, np.ndarray) else v)
        out["returns"] = {"file": a.returns_out, "eps": a.returns_eps, "gamma": a.returns_gamma, "episodes_per_env": a.map_episodes, "decisions_kept": int(m["visits"].sum()),
                          "decisions_cut": int(m["cut_decisions"]), "cells_visited": int((m["visits"] > 0).sum()), "calibration": as_json(summary)}
    if a.split_out:
        import numpy as np
        from dql_multirotor_landing_amd import evaluation, ops
        names = [f for f in ops.SPLIT_FEATURES if f != "coin"] if a.split_by == "all" else [ops.SPLIT_FEATURES[ops.split_feature_code(f)] for f in a.split_by.split(",")]
        m, table = evaluate_split(a.tables, names, n, a.level, flavour=a.flavour, episodes=a.map_episodes, eps=a.split_eps, n_seeds=a.split_seeds, quirks=quirks)
        np.savez_compressed(a.split_out, **m)
        print(evaluation.format_aliasing_table(table), file=sys.stderr)
        out["split"] = {"file": a.split_out, "eps": a.split_eps, "episodes_per_env": a.map_episodes, "seeds": a.split_seeds, "decisions": int(m["pairs_coin"].sum() + m["terminal_coin"].sum()),
                        "table": {k: {f: (v if isinstance(v, int) else round(v, 4)) for f, v in row.items()} for k, row in table.items()}}
    if a.cut_out:
        import numpy as np
        from dql_multirotor_landing_amd import ops
        name = ops.SPLIT_FEATURES[ops.split_feature_code(a.cut_by)]
        cut, visited = evaluate_cut(a.tables, name, n, episodes=a.map_episodes, eps=a.cut_eps, quirks=quirks)
        np.save(a.cut_out, cut)
        out["cut"] = {"file": a.cut_out, "feature": name, "eps": a.cut_eps, "episodes_per_env": a.map_episodes, "states_visited_per_level": visited}
    if a.grid_out:
        import numpy as np
        from dql_multirotor_landing_amd.config import parse_grid_axes
        m, labels, t = evaluate_grid(a.tables, parse_grid_axes(a.grid), n, a.level, flavour=a.flavour, episodes=a.map_episodes, quirks=quirks)
        np.savez_compressed(a.grid_out, **m)
        out["grid"] = {"file": a.grid_out, "scenarios": len(labels), "episodes_per_env": a.map_episodes, "touchdown_rate": [round(float(x), 4) for x in m["rate"]],
                       "labels": labels, "worst_scenario": labels[int(t["worst_scenario"][0])], "worst_touchdown_rate": float(t["worst_rate"][0])}
    out.update({"first_episode_outcomes": h, "touchdown_rate": h["TERMINAL_CONTACT"] / n, "goal_rate": h["TERMINAL_SUCCESS"] / n})
    print(json.dumps(out, indent=1))
