"""raw/*.json[l] -> the table of README.md: per line the parent's and this tree's median and spread.

    python profiles/wg_rank/summary.py profiles/wg_rank/raw"""
import json, statistics as st, sys
d = sys.argv[1]
def load(name, who, i):
    ext = "json" if name in ("track", "vo") else "jsonl"
    return [json.loads(l) for l in open(f"{d}/{name}_{who}_{i}.{ext}") if l.strip().startswith("{")]
def lines(who, i):
    t, v = load("track", who, i)[0], load("vo", who, i)[0]
    g = {r["M"]: r for r in load("guided", who, i) if "M" in r}
    l = load("life", who, i)[0]
    r = {x["batch"]: x for x in load("reloc", who, i)}
    o = {"bench.py default, ms/step": t["ms_per_step"], "bench.py --workload vo, ms/step": v["ms_per_step"]}
    for k in ("stereo_match", "f_lmeds"):
        o[f"  tracking stage {k}, ms"] = t["stage_ms_per_step"][k]
    for k in ("fast", "lk_filter", "right_qs_3d"):
        o[f"  vo stage {k}, ms"] = v["stage_ms_per_step"][k]
    for M in sorted(g):
        for k in ("grid", "track_rows", "steps_1_5"):
            o[f"guided_time M={M} {k}, us"] = g[M]["us"][k]
    for k in ("spawn_with_restore", "compact", "cycle_us"):
        o[f"map_life_time {k}, us"] = l["us"][k] if k in l["us"] else l[k]
    for b in sorted(r):
        o[f"reloc_time batch {b} relocalize, us"] = r[b]["chain_us"]["relocalize"]
        o[f"reloc_time batch {b} map_knn2, us"] = st.median(r[b]["map_knn2_us"])
        assert r[b]["bar_met"], (who, i, b)
    assert l["cycle_le_observe"], (who, i)
    for n, v in load("compact", who, i)[0]["us"].items():
        for k in v:
            o[f"compact_time {k} at {n} entries, us"] = v[k]
    return o
P = [lines("parent", i) for i in (1, 2, 3, 4)]
C = [lines("change", i) for i in (1, 2, 3, 4)]
print("| line | parent median | parent spread (max - min) | this median | this spread | bar (parent median + spread) | verdict |")
print("|---|---|---|---|---|---|---|")
bad = 0
for k in P[0]:
    p, c = [x[k] for x in P], [x[k] for x in C]
    pm, cm, ps, cs = st.median(p), st.median(c), max(p) - min(p), max(c) - min(c)
    ok = cm <= pm + ps
    bad += not ok
    print(f"| {k} | {pm:.4g} | {ps:.3g} | {cm:.4g} | {cs:.3g} | {pm + ps:.4g} | {'met' if ok else 'MISSED'} |")
print("\nlines missed:", bad)
