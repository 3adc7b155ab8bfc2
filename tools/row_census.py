#!/usr/bin/env python3
"""Row census of a locomotion rollout (CPU only: the oracle's fp32 build rolls, its fp64 collide counts).

How much of the step kernel's row work is zero rows: per substep-start state an env has
rows = 3 min(contacts, cap) + limit rows; a wave runs the largest count of its teams (wave_rows), its test solves in
batches of RB columns, its sweeps padded to the prefetch depth PF, and rows past KR from scratch.  The census rolls
the benchmark's kind of rollout (a cycling pool of U(-1, 1) action tensors), sorts each step's envs by a key the way the
work ordering does, and prints the means of wave_rows, batches, remainder columns, padded visits and the waves past KR,
for both substeps.

    python tools/row_census.py --task Ant --num-envs 4096 --pool 8 --first 60 --last 220 --key post

Keys: prev (the previous step's last-substep count: the step kernel's key before round 8), post (the count of the state
the step leaves behind: its key since), ground / limits (post's contact or limit part alone, the other part from
prev), none (unsorted).
"""
import argparse
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "isaacgymenvs-ma_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

KEYS = ("prev", "post", "ground", "limits", "none")


def task_setup(task, n):
    """(spec, sp, tp, mnp, agents) of a locomotion task as make() builds it"""
    from migym import configs, model as M, taskdefs
    cfg = configs.task_config(task, n)
    base = "Ant" if task == "MAAnt" else task
    agents = int(cfg["env"].get("numAgents", 1)) if task == "MAAnt" else 1
    spec = M.load_builtin(taskdefs.TASK_INFO[base][1])
    sp = taskdefs.sim_params(cfg, taskdefs.TASK_INFO[base][5], agents)
    tp = taskdefs.task_params(task, cfg, spec)
    return spec, sp, tp, M.pack_model(spec), agents


def limit_rows(mnp, sp, dof_pos, band=0.0):
    """(rows, near): per env the joint-limit rows build_rows() opens at DOF positions dof_pos (n, nd) -- lower, then
    upper: q - lower < margin, upper - q < margin on limited joints, in fp32 as the kernels compare -- and whether a
    comparison is within `band` of the margin"""
    nd = int(mnp["num_dofs"])
    lim = np.asarray(mnp["limited"][1:nd + 1]) != 0
    lo = np.asarray(mnp["lower"][1:nd + 1], np.float32)
    hi = np.asarray(mnp["upper"][1:nd + 1], np.float32)
    q = np.asarray(dof_pos, np.float32)
    m = np.float32(sp.limit_margin)
    dl, du = q - lo, hi - q
    rows = ((dl < m) & lim).sum(1) + ((du < m) & lim).sum(1)
    near = (((np.abs(dl - m) <= band) | (np.abs(du - m) <= band)) & lim).any(1)
    return rows.astype(np.int32), near


def contact_counts(mnp, sp, root, dof, delta=0.0):
    """(contacts, marked, ground, pairs): per env the oracle's contact count at the thresholds themselves (capped at
    max_contacts like the kernels' lists), whether a candidate lies within delta of its threshold (either side) or
    carries an ambiguity mark (orc_contacts_marks; delta = 0: the plain list, nothing marked), and the count's ground
    and geom-geom parts before the cap"""
    import pyoracle as O
    n = len(root)
    cap = int(sp.max_contacts)
    cnt, mark = np.zeros(n, np.int32), np.zeros(n, bool)
    ground, pairs = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        if delta > 0.0:
            rows, marks, lost = O.contacts_marks(mnp, sp, np.asarray(root[i]).ravel(), dof[i], delta, 64)
            real = (marks & 8) == 0
            mark[i] = lost or bool((marks & (1 | 4 | 8)).any())
            rows = rows[real]
        else:
            rows = O.contacts_full(mnp, sp, np.asarray(root[i]).ravel(), dof[i], 64)
        ground[i] = int((rows[:, 3] < 0).sum())
        pairs[i] = len(rows) - ground[i]
        cnt[i] = min(len(rows), cap)
    return cnt, mark, ground, pairs


def row_counts(mnp, sp, root, dof, delta=0.0, band=0.0):
    """(rows, marginal) of the states: 3 min(contacts, cap) + limit rows, and the envs whose count hangs on a
    comparison within delta (contacts) or band (limits) of its threshold"""
    c, cm, _, _ = contact_counts(mnp, sp, root, dof, delta)
    l, lm = limit_rows(mnp, sp, np.asarray(dof)[:, :, 0], band)
    return 3 * c + l, cm | lm


def half_step(h, mnp, sp, threads):
    """a copy of the host env after the first of the control step's two substeps (orc_simulate_views with
    substeps = 1 and dt / substeps); the actuation is the one env_step's pre_physics left in h.act_eff"""
    g = copy.deepcopy(h)
    s1 = copy.copy(sp)
    s1.dt = sp.dt / sp.substeps
    s1.substeps = 1
    g.simulate(mnp, s1, threads=threads, fp32=True)
    return g


def wave_stats(rows, order, teams, RB, PF, KR, rem=3):
    """per-wave figures of one substep: rows (n,) in dispatch order `order`, `teams` per wave"""
    r = rows[order]
    pad = (-len(r)) % teams
    w = np.pad(r, (0, pad)).reshape(-1, teams).max(1)
    batches = -(-w // RB)
    last = w - (batches - 1) * RB
    short = (w > 0) & (last <= rem)
    prow = -(-w // PF) * PF
    return dict(wave_rows=float(w.mean()), batches=float(batches.mean()), short_last_batch=float(short.mean()),
                padded_visits=float((prow - w).mean()), sweep_rows=float(prow.mean()), past_kr=float((w > KR).mean()))


def census(task="Ant", n=4096, pool=8, first=60, last=220, key="post", seed=0, threads=8, RB=6, PF=4, KR=12,
           out=sys.stdout):
    import pyoracle as O
    spec, sp, tp, mnp, agents = task_setup(task, n)
    na = n * agents
    h = O.HostEnv(tp, spec, na, agents=agents) if agents > 1 else O.HostEnv(tp, spec, na)
    teams = 64 // (16 if int(mnp["num_nodes"]) <= 16 else 32)
    rng = np.random.default_rng(seed)
    acts = rng.uniform(-1, 1, (pool, na, tp.num_actions)).astype(np.float32)
    stats = {1: [], 2: []}
    mix = []
    corr = []
    prev_last = None
    for t in range(last):
        h.actions[:] = acts[t % pool]
        if t >= first:
            pre = copy.deepcopy(h)
            pre.env_step(mnp, sp, tp, seed=seed, step=t, threads=threads, fp32=True)   # act_eff of this step
            g = copy.deepcopy(h)
            g.act_eff[:] = pre.act_eff
            r1, _ = row_counts(mnp, sp, g.root, g.dof)
            c1, _, gr, pr = contact_counts(mnp, sp, g.root, g.dof)
            l1, _ = limit_rows(mnp, sp, g.dof[:, :, 0])
            g2 = half_step(g, mnp, sp, threads)
            r2, _ = row_counts(mnp, sp, g2.root, g2.dof)
            if key == "none" or prev_last is None:
                k = np.zeros(na, np.int32) if key == "none" else r1
            elif key == "prev":
                k = prev_last
            elif key == "post":
                k = r1
            elif key == "ground":
                k = 3 * c1 + (prev_last - 3 * prev_con)
            else:
                k = 3 * prev_con + l1
            if agents > 1:   # an env's agents stay together: the unit's key is its largest
                ku = k.reshape(-1, agents).max(1)
                ou = np.argsort(-ku, kind="stable")
                order = (ou[:, None] * agents + np.arange(agents)[None, :]).ravel()
            else:
                order = np.argsort(-k, kind="stable") if key != "none" else np.arange(na)
            stats[1].append(wave_stats(r1, order, teams, RB, PF, KR))
            stats[2].append(wave_stats(r2, order, teams, RB, PF, KR))
            mix.append((float(r1.mean()), float(r2.mean()), float(gr.mean()), float(pr.mean()), float(l1.mean())))
            if prev_last is not None:
                corr.append((np.corrcoef(prev_last, r1)[0, 1], np.corrcoef(prev_last, r2)[0, 1]))
            prev_last, prev_con = r2, np.minimum(contact_counts(mnp, sp, g2.root, g2.dof)[0], int(sp.max_contacts))
        h.env_step(mnp, sp, tp, seed=seed, step=t, threads=threads, fp32=True)
    m = np.mean(mix, 0)
    print(f"# row census: {task} {n} envs, pool of {pool}, steps {first}..{last - 1}, key {key}, {teams} teams per wave, "
          f"RB {RB}, PF {PF}, KR {KR}", file=out)
    print(f"rows per env: substep 1 {m[0]:.2f}, substep 2 {m[1]:.2f}; ground contacts {m[2]:.2f}, geom pairs {m[3]:.2f}, "
          f"limit rows {m[4]:.2f}", file=out)
    if corr:
        c = np.mean(corr, 0)
        print(f"the previous step's last-substep count correlates {c[0]:.2f} with substep 1's rows, {c[1]:.2f} with "
              f"substep 2's", file=out)
    res = {}
    for s in (1, 2):
        res[s] = {k: float(np.mean([x[k] for x in stats[s]])) for k in stats[s][0]}
        r = res[s]
        print(f"substep {s}: wave_rows {r['wave_rows']:.2f}  batches of {RB} {r['batches']:.2f}  last batch <= 3 rows in "
              f"{100 * r['short_last_batch']:.1f} % of waves  padded visits per sweep {r['padded_visits']:.2f} of "
              f"{r['sweep_rows']:.2f}  waves past KR {100 * r['past_kr']:.1f} %", file=out)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="Ant", choices=["Ant", "MAAnt", "Humanoid"])
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--pool", type=int, default=8, help="action tensors the rollout cycles through (bench.py: 8)")
    ap.add_argument("--first", type=int, default=60, help="first step counted")
    ap.add_argument("--last", type=int, default=220, help="steps rolled (the last one counted is --last - 1)")
    ap.add_argument("--key", default="post", choices=KEYS)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--rb", type=int, default=6)
    ap.add_argument("--kr", type=int, default=12)
    a = ap.parse_args()
    census(a.task, a.num_envs, a.pool, a.first, a.last, a.key, a.seed, a.threads, RB=a.rb, KR=a.kr)


if __name__ == "__main__":
    main()
