"""A sweep of decoder configurations and what prepare() chooses for each: engine, geometry, thread count,
workspace.  tests/golden/engine_choices.json holds the table; test_emu_logic.py (emulator) and
test_gpu_batches.py (HIP library) assert that it is reproduced exactly, and tools/engine_choice_table.py
regenerates it from a given library.

The sweep is built so that every compiled geometry of every lane engine (text_amd/csrc/fltx_engines.h) is chosen
by at least one configuration: `family_counts()` says how many chose each."""
import json
import os

import numpy as np

import cases
import helpers

KEYS = ("engine", "slane", "wlane", "tlane", "xlane", "ylane", "yshare", "lane_groups", "ymemo_slots", "sstream",
        "tstream", "lane", "lean", "threads", "lds", "cap", "cap2", "cut", "recompute", "items", "hot_level", "id_cap",
        "toklm_contexts", "why_not_lane", "ws_bytes")


def _cfg(out, name, c, T=2, B=1, sets=None, stream=False):
    c = dict(c, name=name, T=T)
    out.append(dict(name=name, case=c, B=B, sets=dict(sets or {}), stream=stream))


def _lf(N=29, K=10, Kt=None, crit="ctc", la=False, lm="zero", thr=25.0, u=0):
    return cases.case("lf", N=N, K=K, Kt=Kt, crit=crit, log_add=la, lm=lm, thr=thr, u=u,
                      dist="ctc" if N <= 64 else "uniform", trans_seed=(31 + u % 5) if crit == "asg" else None,
                      lm_weight=0.8 if lm != "zero" else 0.0)


def _lx(K=10, Kt=None, crit="ctc", la=False, lm="zero", lex=cases.SMALL_LEX, scores=None, unk=float("-inf"),
        tok=False, u=0, N=29):
    lex = lex if crit == "ctc" else {cases.SMALL_LEX: cases.NODUP_LEX, cases.MULTI_LEX: cases.MULTI_NODUP_LEX}.get(lex, lex)
    return cases.case("lx", kind="lexicon", dist="lexspell", N=N, K=K, Kt=Kt, crit=crit, log_add=la, lm=lm,
                      lexicon=lex, label_scores=scores, unk_score=unk, is_lm_token=tok, u=u,
                      trans_seed=(41 + u % 5) if crit == "asg" else None, lm_weight=0.7 if lm != "zero" else 0.0,
                      word_score=0.5 if lm != "zero" else 0.0)


TOK_LM = ("ngram", 3, 11)
WORD_LM = ("ngram", 3, 7)


def configs():
    out = []
    # ---- cases of tests/cases.py, truncated to 1 .. 3 frames
    picks = ["lf_ctc_t20_k4", "lf_ctc_t60_k10_kt5", "lf_uni_t40_k10", "lf_ctc_t60_k10_logadd", "lf_ctc_k1", "lf_ctc_thr3",
             "lf_ctc_sil", "lf_asg_t30_n8", "lf_asg_t40_n29_kt7", "lf_ctc_n4", "lf_uni_n40_k20", "lf_uni_n64_k64",
             "lf_ctc_n29_k64", "lf_ctc_n29_k65", "C1_ctc_u0", "C2_ctc_u0", "C2_ctc_u0_kt10", "C2_ctc_u0_logadd",
             "lf_ctc_t300_k100", "lx_spell_t40_k8", "lx_spell_t60_k12_full", "lx_spell_t60_k12_logadd", "lx_spell_unk",
             "lx_uni_t40_k10", "lx_asg_t40", "lx_tokenlm_t40", "lx_scores_t50", "lx_unk_uni_k32", "lx_asg_t40_k24",
             "lx_tokenlm_t80_k24", "ng_word_t40_k10", "ng_word_t60_k16_4g", "ng_word_unk_t40", "ng_word_logadd_t40",
             "ng_tok_lexfree_t40", "ng_tok_lexfree_kt8", "ng_tok_lexicon_t40", "ml_word_t60_k16", "ml_word_uni_t50_k48",
             "ml_word_asg_t40_k24", "ml_word_t80_k100", "ml_word_asg_t80_k200", "hl_lastword_lexfree",
             "hl_lastword_lexfree_kt6_logadd", "hl_lastword_word", "hl_lastword_toklex", "hl_lastword_asg",
             "lx_spell_t60_k32_logadd", "ng_word_logadd_t40_k32", "ml_word_asg_t40_k48", "ng_tok_lexfree_logadd_k16",
             "ng_tok_lexfree_asg_k16", "ng_tok_lexfree_k100", "ng_tok_lexfree_k200_kt8", "ng_tok_lexfree_asg_k300",
             "C3_spell_u0"]
    for i, n in enumerate(picks):
        _cfg(out, "case/%s" % n, cases.BY_NAME[n], T=1 + i % 3)
    # ---- lexicon-free, ZeroLM: beams on both sides of 64 / 128 / 256 / 512, token sets around 64 and word pieces
    for N in (8, 29, 63, 64, 65, 100, 300):
        for K in (1, 63, 64, 65, 128, 129, 256, 257, 512, 513):
            for crit in ("ctc", "asg"):
                if (crit == "asg" and (N > 64 or K in (1, 63, 129, 257, 513))) or (N > 64 and K > 65):
                    continue  # (the generic engine over word pieces at large beams: minutes on the emulator)
                _cfg(out, "lf/N%d/K%d/%s" % (N, K, crit), _lf(N, K, crit=crit, u=N + K))
    # ... fltx_slane.h's (threads, positions) pairs, asked for by thread count; the token-LM variant alike
    for lm in ("zero", TOK_LM):
        tag = "tl" if lm != "zero" else "sl"
        for N, Kt in ((29, None), (29, 31), (40, None), (64, None), (50, None)):
            for st in (0, 320, 384, 448, 512, 576, 640):
                _cfg(out, "%s/N%d/Kt%s/slane_threads%d" % (tag, N, Kt, st), _lf(N, 10, Kt=Kt, lm=lm, u=st),
                     sets={"slane_threads": st} if st else None)
        for thr in (256, 512, 1024):
            _cfg(out, "%s/threads%d" % (tag, thr), _lf(29, 10, lm=lm), sets={"threads": thr})
        for la in (False, True):
            _cfg(out, "%s/la%d/B257" % (tag, la), _lf(29, 16, la=la, lm=lm), T=1, B=257)
            _cfg(out, "%s/la%d/asg" % (tag, la), _lf(29, 16, crit="asg", la=la, lm=lm))
        _cfg(out, "%s/defer" % tag, _lf(29, 16, lm=lm), sets={"defer_check": 1})
        _cfg(out, "%s/defer/slane_threads512" % tag, _lf(29, 16, lm=lm), sets={"defer_check": 1, "slane_threads": 512})
        _cfg(out, "%s/keep_scores" % tag, _lf(29, 16, lm=lm), sets={"keep_scores": 1})
        _cfg(out, "%s/thr_neg" % tag, _lf(29, 16, lm=lm, thr=-1.0))
    for K in (65, 100, 128, 129, 200, 256, 257, 300, 512, 513):
        for N in (29, 40, 64):
            _cfg(out, "tml/N%d/K%d" % (N, K), _lf(N, K, lm=TOK_LM, u=K))
        _cfg(out, "tml/N29/K%d/la" % K, _lf(29, K, la=True, lm=TOK_LM, u=K))
    _cfg(out, "tml/N29/K100/B257", _lf(29, 100, lm=TOK_LM), T=1, B=257)
    _cfg(out, "tml/N29/K100/asg", _lf(29, 100, crit="asg", lm=TOK_LM))
    _cfg(out, "tml/N29/K100/lane_groups-1", _lf(29, 100, lm=TOK_LM), sets={"lane_groups": -1})
    _cfg(out, "tml/N29/K100/lane_groups4", _lf(29, 100, lm=TOK_LM), sets={"lane_groups": 4})
    _cfg(out, "tml/N29/K100/threads512", _lf(29, 100, lm=TOK_LM), sets={"threads": 512})
    _cfg(out, "tml/N29/K100/tok_dense0", _lf(29, 100, lm=TOK_LM), sets={"tok_dense": 0})
    # ---- fltx_mlane.h: every row asked for, lane-group floors
    for geo in range(7):
        for K in (10, 100, 200, 400):
            _cfg(out, "ml/geo%d/K%d" % (geo, K), _lf(29, K, u=geo), sets={"mlane_geo": geo})
        _cfg(out, "ml/geo%d/K100/N40" % geo, _lf(40, 100, u=geo), sets={"mlane_geo": geo})
    for lg in (-1, 2, 4, 8):
        for K in (10, 64, 100, 200):
            _cfg(out, "ml/lane_groups%d/K%d" % (lg, K), _lf(29, K, u=lg), sets={"lane_groups": lg})
    for thr in (640, 768, 960):
        _cfg(out, "ml/threads%d/K200" % thr, _lf(29, 200), sets={"threads": 1024 if thr == 960 else 512})
    _cfg(out, "ml/K100/la", _lf(29, 100, la=True))
    _cfg(out, "ml/K100/B257", _lf(29, 100), T=1, B=257)
    _cfg(out, "ml/K300/N40", _lf(40, 300))
    # ---- fltx_wlane.h: token beams over word-piece sets
    for N in (65, 100, 300):
        for Kt in (5, 30, 35, 36, 50, 56, 57, 64, 65):
            _cfg(out, "wl/N%d/Kt%d" % (N, Kt), _lf(N, 10, Kt=Kt, u=Kt))
    _cfg(out, "wl/la", _lf(100, 10, Kt=30, la=True))
    _cfg(out, "wl/wlane0", _lf(100, 10, Kt=30), sets={"wlane": 0})
    _cfg(out, "wl/threads512", _lf(100, 10, Kt=30), sets={"threads": 512})
    _cfg(out, "wl/K65", _lf(100, 65, Kt=30))
    _cfg(out, "wl/B257", _lf(100, 10, Kt=50), T=1, B=257)
    # ---- streams: fltx_slane.h's stream chunks, with and without a token LM
    for lm in ("zero", TOK_LM):
        tag = "ts" if lm != "zero" else "ss"
        for N, Kt, crit in ((29, None, "ctc"), (29, None, "asg"), (40, None, "ctc"), (64, 40, "ctc"), (29, 10, "ctc")):
            _cfg(out, "%s/N%d/Kt%s/%s" % (tag, N, Kt, crit), _lf(N, 10, Kt=Kt, crit=crit, lm=lm), stream=True)
        _cfg(out, "%s/la" % tag, _lf(29, 10, la=True, lm=lm), stream=True)
        _cfg(out, "%s/K100" % tag, _lf(29, 100, lm=lm), stream=True)
        _cfg(out, "%s/sstream0" % tag, _lf(29, 10, lm=lm), stream=True, sets={"sstream": 0})
        _cfg(out, "%s/B3" % tag, _lf(29, 10, lm=lm), stream=True, B=3)
    _cfg(out, "ts/tlane0", _lf(29, 10, lm=TOK_LM), stream=True, sets={"tlane": 0})
    _cfg(out, "ss/N100", _lf(100, 10, Kt=30), stream=True)
    _cfg(out, "lx/stream", _lx(10), stream=True)
    # ---- fltx_xlane.h
    for Kt in (10, 14, 15, 29):
        for thr in (0, 512, 576, 640):
            _cfg(out, "xl/Kt%d/slane_threads%d" % (Kt, thr), _lx(10, Kt=Kt, u=Kt), sets={"slane_threads": thr})
        _cfg(out, "xl/Kt%d/threads1024" % Kt, _lx(10, Kt=Kt, u=Kt), sets={"threads": 1024})
    for ys in (-1, 0, 1):
        for la in (False, True):
            _cfg(out, "xl/yshare%d/la%d" % (ys, la), _lx(16, la=la), sets={"yshare": ys})
            _cfg(out, "xl/yshare%d/la%d/B257" % (ys, la), _lx(16, la=la), T=1, B=257, sets={"yshare": ys})
    _cfg(out, "xl/K64", _lx(64))
    _cfg(out, "xl/K65", _lx(65))
    _cfg(out, "xl/xlane0", _lx(10), sets={"xlane": 0})
    _cfg(out, "xl/prefer_ylane", _lx(10), sets={"ylane": 2})
    _cfg(out, "xl/unk", _lx(10, unk=-3.0))
    # ---- fltx_ylane.h: LM terms (label scores / word LM), ASG, homophones, logAdd x lane groups x memo place
    for lmk in range(16):
        if lmk & 4 and not lmk & 1:
            continue  # (homophones under ZeroLM: not a lane engine's)
        lm = WORD_LM if lmk & 4 or lmk & 1 and lmk & 2 else "zero"
        scores = (50 + lmk) if lmk & 1 and lm == "zero" else None
        crit = "asg" if lmk & 2 else "ctc"
        lex = cases.MULTI_LEX if lmk & 4 else cases.SMALL_LEX
        for K, ys, yg in ((10, 0, 0), (100, 0, 0), (10, 1, 0), (100, 1, 0), (200, -1, 0), (10, -1, 4), (100, 1, 2)):
            if lmk & 4 and (K > 128 or yg == 4):
                continue
            _cfg(out, "yl/lmk%d/K%d/yshare%d/groups%d" % (lmk, K, ys, yg),
                 _lx(K, crit=crit, la=bool(lmk & 8), lm=lm, lex=lex, scores=scores, u=lmk),
                 sets={"ylane": 2, "yshare": ys, "ylane_groups": yg})
        _cfg(out, "yl/lmk%d/B257" % lmk, _lx(100, crit=crit, la=bool(lmk & 8), lm=lm, lex=lex, scores=scores, u=lmk),
             T=1, B=257)
    for K in (64, 65, 128, 129, 256, 257):
        _cfg(out, "yl/ngram/K%d" % K, _lx(K, lm=WORD_LM, u=K))
    _cfg(out, "yl/long", _lx(100, lm=WORD_LM), T=3)
    _cfg(out, "yl/ylane0", _lx(100, lm=WORD_LM), sets={"ylane": 0})
    _cfg(out, "yl/ylane_asg0", _lx(10, crit="asg", scores=5), sets={"ylane_asg": 0})
    _cfg(out, "yl/threads512/K100", _lx(100, lm=WORD_LM), sets={"threads": 512})
    _cfg(out, "yl/groups4/multi", _lx(100, lm=WORD_LM, lex=cases.MULTI_LEX), sets={"ylane_groups": 4})
    _cfg(out, "yl/unk", _lx(10, lm=WORD_LM, unk=-4.0))
    _cfg(out, "yl/token_lm", _lx(10, lm=TOK_LM, tok=True))
    # ---- the generic engine's switches and host LMs
    for key, val in (("slane", 0), ("lean", 0), ("lane", 0), ("dense", 0), ("force_global_ws", 1), ("cut", 0),
                     ("items", 0), ("slim", 0), ("hot_level", 1), ("lds_budget", 40000), ("cut_m", 200)):
        _cfg(out, "sw/lf/%s%d" % (key, val), _lf(29, 64), sets={key: val})
        _cfg(out, "sw/lx/%s%d" % (key, val), _lx(100, lm=WORD_LM), sets={key: val})
    for K in (10, 100, 200):
        _cfg(out, "hl/lf/K%d" % K, _lf(29, K, lm=("lastword", 5)))
        _cfg(out, "hl/lx/K%d" % K, _lx(K, lm=("lastword", 7)))
    return out


def record(sess, cfg):
    """-> {key: value} after one decode (or one stream chunk) of the configuration, or {"error": <exception class>}."""
    c, B = cfg["case"], cfg["B"]
    inp = helpers.case_inputs(c)
    d = sess.decoder(c, inp)
    try:
        for k, v in cfg["sets"].items():
            d.set(k, v)
        T = [c["T"]] * B
        e = np.ascontiguousarray(np.tile(inp["e"].reshape(-1)[:c["T"] * c["N"]], B), dtype=np.float32)
        if cfg["stream"]:
            d.stream_begin(B, c["N"], 16)
            d.stream_step(e, T)
        else:
            d.decode_batch(e, T, c["N"])
        return {k: int(d.get(k)) for k in KEYS}
    except Exception as ex:  # (a configuration the library refuses is part of the table)
        return {"error": type(ex).__name__}
    finally:
        d.close()


def table(sess):
    return {cfg["name"]: record(sess, cfg) for cfg in configs()}


def golden():
    with open(os.path.join(helpers.GOLDEN_DIR, "engine_choices.json")) as f:
        return json.load(f)


def differences(sess):
    """-> ["<configuration>: <key> <golden> -> <now>", ...] between the committed table and this library's"""
    want, got = golden(), table(sess)
    out = ["%s: only in one table" % k for k in sorted(set(want) ^ set(got))]
    for k in sorted(set(want) & set(got)):
        out += ["%s: %s %s -> %s" % (k, f, want[k].get(f), got[k].get(f))
                for f in sorted(set(want[k]) | set(got[k])) if want[k].get(f) != got[k].get(f)]
    return out


def dumps(tab):
    """the table as JSON, one configuration per line (so that two tables diff line by line)"""
    return "{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(tab[k], sort_keys=True)) for k in sorted(tab)) + "\n}\n"


def _ylane_lmk(c):
    """fltx_ylane.h's LM-term variant of a configuration (prepare(): ylaneLm)"""
    multi = bool(c["lexicon"]) and len(c["lexicon"]) > 2 and "multi" in str(c["lexicon"][2])
    return ((1 if c["lm"] != "zero" or c["label_scores"] is not None else 0) | (2 if c["crit"] == "asg" else 0) |
            (4 if multi else 0) | (8 if c["log_add"] else 0))


def family_counts(tab):
    """-> {family: {geometry: configurations that chose it}} over the lane engines (fltx_ylane.h: every kernel,
    (lane groups, threads, memo in HBM, LMK))"""
    cfg = {c["name"]: c["case"] for c in configs()}
    fam = {}
    for name, r in tab.items():
        if "error" in r:
            continue
        if r["sstream"]:
            f, g = ("tlane_stream" if r["tstream"] else "slane_stream"), (r["sstream"],)
        elif r["ylane"]:
            f, g = "ylane", (r["ylane"], r["threads"], r["yshare"], _ylane_lmk(cfg[name]))
        elif r["xlane"]:
            f, g = "xlane", (r["threads"], r["xlane"])
        elif r["slane"] and r["lane_groups"] > 1:
            f, g = ("tmlane" if r["tlane"] else "mlane"), (r["threads"], r["slane"], r["lane_groups"])
        elif r["slane"]:
            f, g = ("wlane" if r["wlane"] else "tlane" if r["tlane"] else "slane"), (r["threads"], r["slane"])
        else:
            f, g = "generic", (r["engine"],)
        fam.setdefault(f, {}).setdefault(g, 0)
        fam[f][g] += 1
    return fam
