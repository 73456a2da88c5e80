"""Sequential restatement of data::bow_database's two queries (rules 1 to 6) in upstream's own shape: an inverted
file word -> keyframe ids, dicts keyed by keyframe id, and DBoW2's explicit merge loop for the L1 score. Pure Python on purpose: a Python
float is an IEEE f64 and every operation below rounds once, so the scores are the bits rule 1 asks for. Imports nothing of the product."""
import struct


def f32(x):
    """(float)x: narrow an f64 to the nearest f32, returned as the f64 that holds it."""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def score(q, k):
    """DBoW2 L1Scoring::score(q, k) over two {word: value} maps: (score, num_common). The merge loop walks both in ascending word id."""
    qi, ki = sorted(q.items()), sorted(k.items())
    a = b = 0
    s = 0.0
    common = 0
    while a < len(qi) and b < len(ki):
        qw, qv = qi[a]
        kw, kv = ki[b]
        if qw == kw:
            s += abs(qv - kv) - abs(qv) - abs(kv)
            common += 1
            a += 1
            b += 1
        elif qw < kw:
            a += 1   # (DBoW2 jumps with lower_bound; the visited pairs are the same)
        else:
            b += 1
    if common == 0:
        return 0.0, 0
    return -s / 2.0, common


class bow_database:
    def __init__(self):
        self.vecs = {}          # keyframe id -> {word: value}
        self.inverted = {}      # word -> [keyframe ids], in order of registration (upstream: std::list<keyframe*>)

    def add_keyframe(self, kid, bow_vec):
        assert kid not in self.vecs
        self.vecs[kid] = dict(bow_vec)
        for w in bow_vec:
            self.inverted.setdefault(w, []).append(kid)

    def erase_keyframe(self, kid):
        for w in self.vecs.pop(kid):
            self.inverted[w].remove(kid)

    def clear(self):
        self.vecs.clear()
        self.inverted.clear()

    def __len__(self):
        return len(self.vecs)

    def score_all(self, bow_vec):
        """[(keyframe id, num_common, score)] for every registered keyframe, ascending id."""
        return [(kid,) + score(bow_vec, self.vecs[kid])[::-1] for kid in sorted(self.vecs)]

    # ---- rules 2 and 3
    def query(self, bow_vec, reject=()):
        """(survivors [(keyframe id, num_common, score)] ascending id, max_common)."""
        reject = set(reject)
        num_common = {}   # rule 2: the keyframes sharing a word with the query, through the inverted file
        for w in bow_vec:
            for kid in self.inverted.get(w, ()):
                if kid not in reject:
                    num_common[kid] = num_common.get(kid, 0) + 1
        if not num_common:
            return [], 0
        max_common = max(num_common.values())
        thr = f32(f32(0.8) * f32(float(max_common)))   # rule 3, in f32
        out = []
        for kid in sorted(num_common):
            if f32(float(num_common[kid])) > thr:
                out.append((kid, num_common[kid], score(bow_vec, self.vecs[kid])[0]))
        return out, max_common

    # ---- rules 4 to 6; `trace`, if a dict, receives what every gate dropped
    def _candidates(self, bow_vec, reject, top_covisibilities, min_score, trace=None):
        survivors, max_common = self.query(bow_vec, reject)
        if trace is not None:
            reject_set = set(reject)
            initial = [kid for kid in sorted(self.vecs) if kid not in reject_set and score(bow_vec, self.vecs[kid])[1] >= 1]
            trace["initial"] = initial
            trace["dropped_gate3"] = [kid for kid in initial if kid not in {s[0] for s in survivors}]
        scores = {}   # rule 4: the score narrowed to f32
        dropped4 = []
        for kid, _, sc in survivors:
            sc = f32(sc)
            if sc >= f32(min_score):
                scores[kid] = sc
            else:
                dropped4.append(kid)
        if trace is not None:
            trace["dropped_gate4"] = dropped4
        if not scores:
            if trace is not None:
                trace["dropped_gate6"] = []
            return []
        records = []   # rule 5
        best_total = 0.0
        first = True
        for c in sorted(scores):
            total = scores[c]
            best = c
            for n in list(top_covisibilities(c))[:10]:
                if n not in scores:
                    continue
                total = f32(total + scores[n])
                if scores[best] < scores[n]:
                    best = n
            records.append((total, best))
            if first or best_total < total:
                best_total = total
                first = False
        thr = f32(f32(0.75) * best_total)   # rule 6
        out = []
        dropped6 = []
        for total, best in records:
            if total > thr:
                if best not in out:
                    out.append(best)
            else:
                dropped6.append(best)
        if trace is not None:
            trace["dropped_gate6"] = dropped6
        return out

    def acquire_loop_candidates(self, qry_id, bow_vec, connected_ids, top_covisibilities, min_score, trace=None):
        return self._candidates(bow_vec, [qry_id] + list(connected_ids), top_covisibilities, min_score, trace)

    def acquire_relocalization_candidates(self, bow_vec, top_covisibilities, trace=None):
        return self._candidates(bow_vec, [], top_covisibilities, 0.0, trace)
