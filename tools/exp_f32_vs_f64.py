"""float32 HIP kernel vs float64 oracle from identical states, per field, over 1 period and over a 16-period launch, on the config
flavours the throughput figures run on.  Prints one JSON line per (case, periods): max error per field group —
the numbers tests/test_gpu_parity.py's tolerances are set from.  usage: python tools/exp_f32_vs_f64.py [n_envs]

`python tools/exp_f32_vs_f64.py flavours [oracle|hip]`: the flavours of tests/f32_step_checks.py instead (simulation / training at levels 2 and 4, paper
mode, greedy on the stage-4 tables, handed over so that the 16 periods contain the episode ends), one period per call, with the float32 CPU oracle
(default: needs no GPU; it is bit-identical to the kernel) or the HIP engine as the float32 side; then the G13 flights in float32 against the recording:
max error per signal column, and the bound the tests assert (4 x the maximum, rounded up to one significant digit).  -> profiles/f32_step_vs_f64_flavours.jsonl

`python tools/exp_f32_vs_f64.py episodes [out.jsonl]`: whole first episodes of 4 096 envs in float32 against their float64 twins on the CPU oracle, greedy on the
stage-4 tables, for every flavour and seed of tests/episode_dtype_checks.py (needs no GPU): per pair the decision counts, the terminal codes, McNemar's
counts, the paired means, the maxima per field group at the terminal of the decision-concordant envs and those envs' mean difference of the return; then
the two tables of bounds that module asserts.
-> profiles/f32_episodes_vs_f64.jsonl"""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dql_multirotor_landing_amd.config import CHECK_NAMES, DqlConfig, F32, F64  # noqa: E402
from dql_multirotor_landing_amd.engine import Engine  # noqa: E402
from dql_multirotor_landing_amd.state_layout import to_f32_filter_state  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

CASES = {
    "default": {},
    "configs4": dict(per_env_platform=1, noise_pos_sd=0.25, noise_vel_sd=0.1),
    "two_axis": dict(two_axis=1),
    "two_axis_configs4": dict(two_axis=1, per_env_platform=1, noise_pos_sd=0.25, noise_vel_sd=0.1),
}
GROUPS = {
    "pose": ["px", "py", "pz", "qw", "qx", "qy", "qz"], "vel": ["vx", "vy", "vz", "wx", "wy", "wz"], "rotor": ["om0", "om1", "om2", "om3"],
    "pid": ["vz_i", "yw_i", "vz_state", "yw_state"], "platform": ["mp_phase", "mp_x", "mp_u", "mp_y", "mp_v"],
    "obs_pv": ["obs_p_x", "obs_v_x", "obs_p_y", "obs_v_y"], "obs_a": ["obs_a_x", "obs_a_y", "kal_x_x", "kal_y_x"], "kal_P": ["kal_x_P", "kal_y_P"],
    "reward": ["reward"], "cum": ["cum_x", "cum_y"], "shaping": ["shp_x_p", "shp_x_v", "shp_x_a", "shp_y_p", "shp_y_v", "shp_y_a"], "sp": ["pitch_sp", "roll_sp"],
}


def one_digit_up(x):
    """x rounded up to one significant digit"""
    import math
    if x == 0.0:
        return 0.0
    e = math.floor(math.log10(x))
    return float(f"{math.ceil(x / 10 ** e - 1e-12) * 10.0 ** e:.1g}")


def flavours(side):
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
    import f32_step_checks as sc
    make = (lambda cfg, n, seed: Engine(cfg, n, seed=seed)) if side == "hip" else (lambda cfg, n, seed: Oracle(cfg, n, seed=seed, n_threads=16))
    for name in sc.FLAVOURS:
        res = sc.fly(make, name)
        n = len(res["alive"][0])
        for k, groups in sc.measured(res).items():
            row = {"flavour": name, "f32_side": side, "periods": k, "n": n, "handover_period": sc.FLAVOURS[name][2],
                   "envs_left_comparison": n - int(res["alive"][k - 1].sum()), "episode_ends_by_code_in_window": res["ended"].tolist(),
                   "envs_touched_down_in_window": int(res["contact_envs"].sum())}
            if sc.acc_is_difference_quotient(res["cfg"]):
                r32, _, r64, _ = res["snap"][k]
                row["acc_pair_worst_fraction_of_its_bound"] = max(
                    float((np.abs(r32[res["names"].index(f)] - r64[res["names"].index(f)]) / sc.acc_bound(res["cfg"], r64, res["names"], sc.TOL[k][0], f))[res["alive"][k - 1]].max())
                    for f in sc._ACC)
            row.update(groups)
            print(json.dumps(row), flush=True)
    z = np.load(sc.GOLDEN / "g13_env.npz")
    worst = np.zeros(len(sc.G13_SIGNALS))
    big = {k: np.inf for k in sc.G13_SIGNALS}
    for tag in sc.G13_CASES:
        sig, out = sc.g13_fly(make, tag, z)
        err, rew = sc.check_g13_flight(tag, z, sig, out, bounds=big)
        worst = np.maximum(worst, err)
        print(json.dumps({"g13": tag, "f32_side": side, "periods": len(sig), "max_abs_vs_recording": dict(zip(sc.G13_SIGNALS, err.tolist())), "reward_max_abs": rew}), flush=True)
    print(json.dumps({"g13": "all", "f32_side": side, "max_abs_vs_recording": dict(zip(sc.G13_SIGNALS, worst.tolist())),
                      "asserted_bound_4x_one_digit_up": {k: one_digit_up(4 * w) for k, w in zip(sc.G13_SIGNALS, worst.tolist())}}), flush=True)


def episodes(out_path):
    import time
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
    import episode_dtype_checks as ec
    import rollout_checks as rc
    make = lambda cfg, n, seed: Oracle(cfg, n, seed=seed, n_threads=16)
    tables = rc.stage4_tables()
    lines = []
    for name, (make_cfg, kind) in ec.FLAVOURS.items():
        for seed in ec.SEEDS:
            t0 = time.perf_counter()
            pair = ec.paired_flights(make, make_cfg, tables, ec.N_ENVS, seed, ec.MAX_STEPS)
            seconds = time.perf_counter() - t0
            m = ec.compare(pair)
            bal = ec.balance(pair, kind, make_cfg(F64).two_axis, ~m["concordant"])
            b, c = bal["landing_f32_only"], bal["landing_f64_only"]
            row = {"flavour": name, "seed": seed, "n": m["n"], "max_steps": ec.MAX_STEPS, "f32_side": "oracle", "seconds_for_the_pair": round(seconds, 2),
                   "f64_terminal_codes": rc.histogram(pair[F64]["code"]), "envs_with_a_differing_decision": m["discordant_envs"],
                   "differing_period_slots": m["differing_slots"], "f64_periods_flown": m["f64_periods_flown"],
                   "envs_with_a_differing_decision_while_both_fly": m["discordant_while_both_fly"], "terminal_code_differs": m["terminal_code_differs"],
                   "concordant_envs_with_another_code_or_step_count": int(m["strict_exceptions"].size), "landing_outcome": CHECK_NAMES[ec.landing_code(kind)],
                   "landing_f32_only": b, "landing_f64_only": c, "mcnemar_z": (abs(b - c) / (b + c) ** 0.5 if b + c else 0.0),
                   "paired_mean_standard_error_and_flights_that_part": bal["paired"], "paired_mean_z": {f: (abs(v[0]) / v[1] if v[1] else 0.0) for f, v in bal["paired"].items()},
                   "paired_mean_z_of_all_pairs_unasserted": {f: (abs(v[0]) / v[1] if v[1] else 0.0) for f, v in bal["paired_raw"].items()},
                   "max_abs_at_terminal": m["max_abs_at_terminal"], "max_abs_per_field": m["max_abs_per_field"],
                   "concordant_mean_difference": m["concordant_mean_difference"], "concordant_return_difference_vs_terminal_offset": ec.return_vs_offset(pair, m, make_cfg(F64))}
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    Path(out_path).write_text("\n".join(lines) + "\n")
    bounds, _ = ec.bounds_from_profile(out_path)
    print("episode_dtype_checks.BOUNDS (4 x the maxima, one digit up):", bounds, flush=True)
    print("episode_dtype_checks.CONCORDANT_MEAN_BOUNDS (4 x the larger seed, one digit up):", ec.concordant_mean_bounds_from_profile(out_path), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "flavours":
        return flavours(sys.argv[2] if len(sys.argv) > 2 else "oracle")
    if len(sys.argv) > 1 and sys.argv[1] == "episodes":
        return episodes(sys.argv[2] if len(sys.argv) > 2 else Path(__file__).resolve().parent.parent / "profiles" / "f32_episodes_vs_f64.jsonl")
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    for case, kw in CASES.items():
        for periods in (1, 16):
            o64 = Oracle(DqlConfig(dtype=F64, **kw), n, seed=9, n_threads=16)
            o64.train_steps(50, 1.0)
            reals, ints = o64.get_fields()
            e32 = Engine(DqlConfig(dtype=F32, **kw), n, seed=9)
            e32.train_steps(50, 1.0)
            names = e32.field_names()
            qa, qb, cnt = o64.qa.copy(), o64.qb.copy(), o64.count.copy()
            e32.set_tables(qa, qb, cnt); o64.set_tables(qa, qb, cnt)
            e32.set_fields(to_f32_filter_state(reals, names), ints)
            e32.set_option("periods_per_launch", periods); o64.set_option("periods_per_launch", periods)
            e32.train_steps(periods, 1.0); o64.train_steps(periods, 1.0)
            r32, i32 = e32.get_fields(); r64, i64 = o64.get_fields()
            inames = e32.field_names(True)
            same = np.ones(n, dtype=bool)
            for k in ("step_count", "code", "flags", "cur_check"):
                same &= i32[inames.index(k)] == i64[inames.index(k)]
            row = {"case": case, "periods": periods, "n": n, "envs_with_same_episode_state": float(same.mean()),
                   "idx_x_mismatch": float((i32[0] != i64[0])[same].mean()), "idx_y_mismatch": float((i32[1] != i64[1])[same].mean()),
                   "resets_in_window": float(((i64[inames.index("flags")] & 8) != 0).mean())}
            for g, fields in GROUPS.items():
                worst_abs, worst_rel = 0.0, 0.0
                for f in fields:
                    k = names.index(f)
                    d = np.abs(r32[k] - r64[k])[same]
                    if d.size == 0:
                        continue
                    worst_abs = max(worst_abs, float(d.max()))
                    worst_rel = max(worst_rel, float((d / np.maximum(np.abs(r64[k][same]), 1.0)).max()))
                row[g] = [worst_abs, worst_rel]
            print(json.dumps(row), flush=True)
            e32.close()


if __name__ == "__main__":
    main()
