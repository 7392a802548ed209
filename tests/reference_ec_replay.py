"""Replays a request of tests/reference_ec_cases.py through the project's own code and gives the answers in the
driver's form, so that they compare with the record (tests/golden/reference_ec.json) by plain equality.

Two subjects: the oracle's restatement (oracle/ec_ref.py for bytes and matrices, oracle/plan_ref.py for partitions,
flags and plans) and the product's ErasureCode facade (ecg.py), on numpy blocks (host tier) or torch ones (device tier).
"""
import hashlib

import numpy as np

import reference_ec_cases as C


class HostBlocks:
    """numpy blocks: the facade's host tier, and all the oracle takes."""

    @staticmethod
    def zeros(B):
        return np.zeros(B, np.uint8)

    @staticmethod
    def load(raw):
        return np.frombuffer(raw, np.uint8).copy()

    @staticmethod
    def clone(b):
        return b.copy()

    @staticmethod
    def raw(b):
        return b.tobytes()

    @staticmethod
    def raws(blocks):
        return [b.tobytes() for b in blocks]


class DeviceBlocks:
    """torch uint8 tensors on cuda:0: the facade's device tier."""

    @staticmethod
    def zeros(B):
        import torch
        return torch.zeros(B, dtype=torch.uint8, device="cuda:0")

    @staticmethod
    def load(raw):
        import torch
        return torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to("cuda:0")

    @staticmethod
    def clone(b):
        return b.clone()

    @staticmethod
    def raw(b):
        return b.cpu().numpy().tobytes()

    @staticmethod
    def raws(blocks):  # one copy back for the whole stripe
        import torch
        return [row.tobytes() for row in torch.stack(blocks).cpu().numpy()]


def entry(raw):
    return [hashlib.sha256(raw).hexdigest(), raw[:16].hex()]


def plan_form(plans):
    return [[int(bool(p.local_or_column)), [int(x) for x in p.failure_idxs], [[int(b) for b in h] for h in p.help_blocks]]
            for p in plans]


class OracleSubject:
    def __init__(self, inst):
        from oracle import ec_ref as E
        from oracle import plan_ref as P
        t, q = inst["type"], inst["params"]
        self.inst = inst
        self.ec = E.ec_factory(t, E.CodingParameters(**q))
        self.ec.init_coding_parameters(E.CodingParameters(**q))
        if t == 8:
            self.ec.isvertical = bool(inst["isvertical"])
        self.pl = P.planner_for(C.TYPE_NAMES[t], q)

    def matrix(self):
        return self.ec.make_encoding_matrix() if hasattr(self.ec, "make_encoding_matrix") else None

    def partition(self, rule):
        self.pl.placement_rule = 0 if rule == "F" else 2
        return self.pl.generate_partition()

    def decodable(self, fails):
        if hasattr(self.pl, "check_if_decodable"):
            return self.pl.check_if_decodable(list(fails))
        return self.pl.generate_repair_plan(list(fails))[0]  # the product codes' planner stops where the check does

    def plan(self, fails):
        ret, plans = self.pl.generate_repair_plan(list(fails))
        self.pl.local_or_column = False
        return ret, plan_form(plans)

    def set_local(self, loc):
        self.ec.local_or_column = bool(loc)


class FacadeSubject:
    def __init__(self, inst):
        import ecg
        self.ecg, self.inst = ecg, inst
        self.ec = ecg.ec_factory(inst["type"], ecg.CodingParameters(**inst["params"]))
        self.set_local(0)

    def set_local(self, loc):
        self.ec.init_coding_parameters(self.ecg.CodingParameters(**self.inst["params"], local_or_column=bool(loc)))
        if self.inst["type"] == 8:
            self.ec.set_isvertical(bool(self.inst["isvertical"]))

    def matrix(self):
        return None if self.inst["type"] >= 7 else self.ec.make_encoding_matrix()

    def partition(self, rule):
        self.ec.placement_rule = self.ecg.PlacementRule.FLAT if rule == "F" else self.ecg.PlacementRule.OPTIMAL
        return self.ec.generate_partition()

    def decodable(self, fails):
        return self.ec.check_if_decodable(list(fails))

    def plan(self, fails):
        ret, plans = self.ec.generate_repair_plan(list(fails))
        self.set_local(0)
        return ret, plan_form(plans)


def _take(words, at):
    n = int(words[at])
    return [int(x) for x in words[at + 1:at + 1 + n]], at + 1 + n


def stripe_of(subject, inp, B, mem=HostBlocks):
    """The k data blocks cut from the input and the m parities the subject's encode gives them."""
    ec = subject.ec
    blocks = [mem.load(C.data_block(inp, i, B)) for i in range(ec.k)]
    blocks += [mem.zeros(B) for _ in range(ec.m)]
    rc = ec.encode(blocks[:ec.k], blocks[ec.k:], B)
    assert rc in (None, 0), rc
    return blocks


def replay(subject, lines, inp, with_bytes=True, stripes=None, mem=HostBlocks):
    """One answer per line, in the driver's form.  with_bytes=False leaves out everything that moves block bytes (a
    line that does nothing else answers None); stripes (size -> blocks) is filled by the encodes and may be handed on to a later
    call; mem says where the blocks live."""
    ec = subject.ec
    stripes = {} if stripes is None else stripes
    rule = None
    out = []
    for line in lines:
        w = line.split()
        op = w[0]
        if op == "code":
            out.append({"k": ec.k, "m": ec.m})
        elif op == "mat":
            out.append({"matrix": subject.matrix()})
        elif op == "part":
            rule = w[1]
            out.append({"partition": subject.partition(rule)})
        elif not with_bytes and op != "pat":
            out.append(None)
        elif op == "enc":
            B = int(w[1])
            stripes[B] = stripe_of(subject, inp, B, mem)
            out.append({"out": [entry(mem.raw(b)) for b in stripes[B][ec.k:]]})
        elif op == "add":
            B, bn, pn = int(w[1]), int(w[2]), int(w[3])
            res = [mem.zeros(B) for _ in range(pn)]
            ec.perform_addition(stripes[B][:bn], res, B, bn, pn)
            out.append({"out": [entry(mem.raw(b)) for b in res]})
        elif op == "pat":
            if w[1] != rule:
                rule = w[1]
                subject.partition(rule)
            fails, _ = _take(w, 3)
            dec = bool(subject.decodable(fails))
            ret, plans = subject.plan(fails)
            r = {"dec": int(dec), "ret": int(bool(ret)), "plans": plans}
            if with_bytes:
                r["d"] = {}
                for bit, B in enumerate(C.SIZES):
                    if not dec or not int(w[2]) >> bit & 1:
                        continue
                    blocks = [mem.clone(b) for b in stripes[B]]
                    for f in fails:
                        blocks[f][:] = C.ERASED
                    n = len(blocks)
                    ec.decode(blocks[:ec.k], blocks[ec.k:], B, list(fails) + [-1] * (n + 1 - len(fails)), len(fails))
                    raws = mem.raws(blocks)
                    r["d"][str(B)] = {"out": [entry(raws[f]) for f in fails],
                                      "all": hashlib.sha256(b"".join(raws)).hexdigest()}
            out.append(r)
        elif op in ("pdec", "penc"):
            B, loc = int(w[1]), int(w[2])
            a, at = _take(w, 3)
            b, at = _take(w, at)
            c = _take(w, at)[0] if op == "pdec" else None
            res = [mem.zeros(B) for _ in range(len(c if op == "pdec" else b))]
            subject.set_local(loc)
            data = [stripes[B][i] for i in a]
            if op == "pdec":
                ec.encode_partial_blocks_for_decoding(data, res, B, a, b, c)
            else:
                ec.encode_partial_blocks_for_encoding(data, res, B, a, b)
            subject.set_local(0)
            out.append({"out": [entry(mem.raw(x)) for x in res]})
        else:
            raise ValueError(line)
    return out


def partial_matrix_outputs(facade, oracle_ref, line, stripes):
    """What the facade's partial_decoding_matrix / partial_encoding_matrix coefficients make of a pdec / penc line's
    input blocks, through the oracle's plain matrix encode: the bytes those coefficients imply."""
    w = line.split()
    B, loc = int(w[1]), int(w[2])
    a, at = _take(w, 3)
    b, at = _take(w, at)
    facade.set_local(loc)
    if w[0] == "pdec":
        c = _take(w, at)[0]
        M, rows = facade.ec.partial_decoding_matrix(a, b, c), len(c)
    else:
        M, rows = facade.ec.partial_encoding_matrix(a, b), len(b)
    facade.set_local(0)
    res = [np.zeros(B, np.uint8) for _ in range(rows)]
    oracle_ref.jerasure_matrix_encode(len(a), rows, M, [stripes[B][i] for i in a], res, B)
    return {"out": [entry(x.tobytes()) for x in res]}


def request_of(inst, subject, inp, stripes=None, with_bytes=True):
    """(lines, answers to the head and pattern lines): the code's request with the partial lines the subject's own plans
    give.  It is the recorded request only if those plans are the reference's (the record keeps the request's digest)."""
    base = C.head_lines(inst) + C.pattern_lines(inst)
    answers = replay(subject, base, inp, with_bytes=with_bytes, stripes=stripes)
    return C.code_lines(inst, answers), answers


def folded(inst, lines, answers):
    """The answers in the record's form, "reference_exits" where the record says the reference ended its process."""
    return C.fold(lines, ["reference_exits" if i in inst["exits"] else a for i, a in enumerate(answers)])
