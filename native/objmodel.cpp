// _objmodel: native object-model core (kube/objects.py, kube/informer.py).
//
// Every reconcile, apiserver write and informer event passes through a few
// small helpers many times per claim: metadata and condition accessors, the
// RFC 3339 timestamp, uid generation, quantity arithmetic and the informer's
// index bookkeeping. This module implements them against the raw CPython C
// API, as jsontree.cpp does for the tree walks.
//
//   name_of ... object_key        accessors over wire-format dicts
//   set_condition                 metav1.Condition upsert
//   fmt_time, fmt_micro_time      RFC 3339 for datetimes whose tzinfo is utc
//   now_rfc3339, uuid4_str        cached clock string, OS-random uuid
//   qty_parse, qty_fmt, qty_addsub
//                                 exact quantity arithmetic on (num, den)
//   field_index, index_store      informer indexer and store update
//
// The pure-Python functions stay in the package as the fallback and as the
// reference the tests compare against. The fast paths mirror them for the
// shapes the wire format has (exact dict/list/str); on anything else the
// call is handed to the Python body unchanged (bound with set_fallbacks), so
// odd input behaves, and raises, exactly as before.
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <datetime.h>

#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/random.h>
#include <time.h>

namespace {

struct Names {
    PyObject *metadata, *name, *namespace_, *uid, *labels, *annotations, *finalizers,
        *deletionTimestamp, *ownerReferences, *spec, *providerID, *status, *conditions,
        *type, *reason, *message, *lastTransitionTime, *observedGeneration, *generation,
        *Ready, *True_, *empty, *at;
} S;

PyObject* long_zero;
PyObject* long_thousand;

// ---------------------------------------------------------------------------
// Python bodies the fast paths defer to
// ---------------------------------------------------------------------------

enum Fn {
    F_NAME_OF, F_NAMESPACE_OF, F_UID_OF, F_LABELS_OF, F_ANNOTATIONS_OF, F_FINALIZERS_OF,
    F_HAS_FINALIZER, F_IS_DELETING, F_OWNER_REFERENCES_OF, F_PROVIDER_ID_OF, F_NODE_IS_READY,
    F_NODE_READY_CONDITION, F_GET_CONDITION, F_CONDITION_IS, F_CONDITION_IS_TRUE,
    F_SET_CONDITION, F_FMT_TIME, F_FMT_MICRO_TIME, F_OBJECT_KEY, F_COUNT
};

const char* const fn_names[F_COUNT] = {
    "name_of", "namespace_of", "uid_of", "labels_of", "annotations_of", "finalizers_of",
    "has_finalizer", "is_deleting", "owner_references_of", "provider_id_of", "node_is_ready",
    "node_ready_condition", "get_condition", "condition_is", "condition_is_true",
    "set_condition", "fmt_time", "fmt_micro_time", "object_key",
};

PyObject* fallback[F_COUNT];

PyObject* defer(int fn, PyObject* const* args, Py_ssize_t nargs, PyObject* kwnames = nullptr) {
    if (fallback[fn] == nullptr) {
        PyErr_Format(PyExc_RuntimeError, "_objmodel: no Python body bound for %s", fn_names[fn]);
        return nullptr;
    }
    return PyObject_Vectorcall(fallback[fn], args, (size_t)nargs, kwnames);
}

PyObject* py_set_fallbacks(PyObject*, PyObject* table) {
    if (!PyDict_Check(table)) {
        PyErr_SetString(PyExc_TypeError, "set_fallbacks(table) takes a dict of name -> function");
        return nullptr;
    }
    for (int i = 0; i < F_COUNT; i++) {
        PyObject* f = PyDict_GetItemString(table, fn_names[i]);  // borrowed
        if (f == nullptr) continue;
        Py_INCREF(f);
        Py_XSETREF(fallback[i], f);
    }
    Py_RETURN_NONE;
}

// ---------------------------------------------------------------------------
// lookups
// ---------------------------------------------------------------------------

// d.get(key) on an exact dict: 1 found (*out borrowed), 0 absent, -1 error
inline int look(PyObject* d, PyObject* key, PyObject** out) {
    *out = PyDict_GetItemWithError(d, key);
    if (*out != nullptr) return 1;
    return PyErr_Occurred() ? -1 : 0;
}

// obj.get(key, {}) where both must be exact dicts: 1 found, 0 absent,
// -1 error, -2 not a shape the fast path mirrors
inline int section(PyObject* obj, PyObject* key, PyObject** out) {
    if (!PyDict_CheckExact(obj)) return -2;
    int r = look(obj, key, out);
    if (r == 1 && !PyDict_CheckExact(*out)) return -2;
    return r;
}

// a == b for the values conditions hold: exact str or None on both sides.
// 1 equal, 0 not equal, -2 anything else (Python's == decides).
inline int fast_eq(PyObject* a, PyObject* b) {
    bool sa = PyUnicode_CheckExact(a), sb = PyUnicode_CheckExact(b);
    if (sa && sb) return a == b || PyUnicode_Compare(a, b) == 0;
    if ((sa || a == Py_None) && (sb || b == Py_None)) return a == b;
    return -2;
}

// ---------------------------------------------------------------------------
// metadata / spec accessors
// ---------------------------------------------------------------------------

enum Kind { K_STR, K_OR_DICT, K_OR_LIST, K_BOOL };

// obj.get(sec, {}).get(key, "") | .get(key) or {} | .get(key) or [] | bool(.get(key))
PyObject* field(int fn, PyObject* obj, PyObject* sec_key, PyObject* key, Kind kind) {
    PyObject* sec;
    int r = section(obj, sec_key, &sec);
    if (r == -1) return nullptr;
    if (r == -2) return defer(fn, &obj, 1);
    PyObject* v = nullptr;
    if (r == 1 && look(sec, key, &v) < 0) return nullptr;
    if (kind == K_STR) {
        if (v == nullptr) v = S.empty;
        Py_INCREF(v);
        return v;
    }
    int truth = 0;
    if (v != nullptr) {
        Py_INCREF(v);
        truth = PyObject_IsTrue(v);
        if (truth <= 0) Py_DECREF(v);
        if (truth < 0) return nullptr;
    }
    if (kind == K_BOOL) {
        if (truth) Py_DECREF(v);
        return PyBool_FromLong(truth);
    }
    if (truth) return v;
    return kind == K_OR_DICT ? PyDict_New() : PyList_New(0);
}

#define ACCESSOR(cname, fn, sec, key, kind) \
    PyObject* cname(PyObject*, PyObject* obj) { return field(fn, obj, S.sec, S.key, kind); }

ACCESSOR(py_name_of, F_NAME_OF, metadata, name, K_STR)
ACCESSOR(py_namespace_of, F_NAMESPACE_OF, metadata, namespace_, K_STR)
ACCESSOR(py_uid_of, F_UID_OF, metadata, uid, K_STR)
ACCESSOR(py_labels_of, F_LABELS_OF, metadata, labels, K_OR_DICT)
ACCESSOR(py_annotations_of, F_ANNOTATIONS_OF, metadata, annotations, K_OR_DICT)
ACCESSOR(py_finalizers_of, F_FINALIZERS_OF, metadata, finalizers, K_OR_LIST)
ACCESSOR(py_owner_references_of, F_OWNER_REFERENCES_OF, metadata, ownerReferences, K_OR_LIST)
ACCESSOR(py_is_deleting, F_IS_DELETING, metadata, deletionTimestamp, K_BOOL)
ACCESSOR(py_provider_id_of, F_PROVIDER_ID_OF, spec, providerID, K_STR)

PyObject* py_has_finalizer(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    PyObject* sec;
    int r = nargs == 2 ? section(args[0], S.metadata, &sec) : -2;
    if (r == -1) return nullptr;
    if (r == -2) return defer(F_HAS_FINALIZER, args, nargs);
    PyObject* fins = nullptr;
    if (r == 1 && look(sec, S.finalizers, &fins) < 0) return nullptr;
    if (fins == nullptr) Py_RETURN_FALSE;  // fin in []
    Py_INCREF(fins);
    int truth = PyObject_IsTrue(fins);
    int in = truth > 0 ? PySequence_Contains(fins, args[1]) : truth;
    Py_DECREF(fins);
    if (in < 0) return nullptr;
    return PyBool_FromLong(in);
}

// f"{ns}/{name}" if ns else name
PyObject* py_object_key(PyObject*, PyObject* obj) {
    PyObject* sec;
    int r = section(obj, S.metadata, &sec);
    if (r == -1) return nullptr;
    if (r == -2) return defer(F_OBJECT_KEY, &obj, 1);
    PyObject *ns = nullptr, *name = nullptr;
    if (r == 1 && (look(sec, S.namespace_, &ns) < 0 || look(sec, S.name, &name) < 0)) return nullptr;
    if (ns == nullptr) ns = S.empty;
    if (name == nullptr) name = S.empty;
    if (!PyUnicode_CheckExact(ns) || !PyUnicode_CheckExact(name)) return defer(F_OBJECT_KEY, &obj, 1);
    if (PyUnicode_GET_LENGTH(ns) == 0) {
        Py_INCREF(name);
        return name;
    }
    return PyUnicode_FromFormat("%U/%U", ns, name);
}

// ---------------------------------------------------------------------------
// conditions
// ---------------------------------------------------------------------------

// first c in (obj.get("status", {}).get("conditions") or []) with
// c.get("type") == cond_type. 1 found (*out borrowed), 0 none, -1 error,
// -2 defer. Nothing here runs Python code, so borrowed references hold.
int find_condition(PyObject* obj, PyObject* cond_type, PyObject** out) {
    PyObject* st;
    int r = section(obj, S.status, &st);
    if (r <= 0) return r;
    PyObject* conds;
    r = look(st, S.conditions, &conds);
    if (r <= 0) return r;
    if (conds == Py_None) return 0;
    if (!PyList_CheckExact(conds)) return -2;
    for (Py_ssize_t i = 0; i < PyList_GET_SIZE(conds); i++) {
        PyObject* c = PyList_GET_ITEM(conds, i);
        if (!PyDict_CheckExact(c)) return -2;
        PyObject* t;
        if (look(c, S.type, &t) < 0) return -1;
        int e = fast_eq(t != nullptr ? t : Py_None, cond_type);
        if (e == -2) return -2;
        if (e) {
            *out = c;
            return 1;
        }
    }
    return 0;
}

// c.get("status") == status for a found condition: 1, 0, -1 error, -2 defer
int status_is(PyObject* c, PyObject* status) {
    PyObject* st;
    if (look(c, S.status, &st) < 0) return -1;
    return fast_eq(st != nullptr ? st : Py_None, status);
}

PyObject* get_condition(int fn, PyObject* const* args, Py_ssize_t nargs, PyObject* cond_type) {
    PyObject* c;
    int r = find_condition(args[0], cond_type, &c);
    if (r == -1) return nullptr;
    if (r == -2) return defer(fn, args, nargs);
    if (r == 0) Py_RETURN_NONE;
    Py_INCREF(c);
    return c;
}

PyObject* py_get_condition(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 2) return defer(F_GET_CONDITION, args, nargs);
    return get_condition(F_GET_CONDITION, args, nargs, args[1]);
}

PyObject* py_node_ready_condition(PyObject*, PyObject* node) {
    return get_condition(F_NODE_READY_CONDITION, &node, 1, S.Ready);
}

// bool(c) and c.get("status") == status
PyObject* condition_is(int fn, PyObject* const* args, Py_ssize_t nargs, PyObject* status,
                       bool need_nonempty) {
    PyObject* c;
    int r = find_condition(args[0], nargs > 1 ? args[1] : S.Ready, &c);
    if (r == 1) r = (need_nonempty && PyDict_GET_SIZE(c) == 0) ? 0 : status_is(c, status);
    if (r == -1) return nullptr;
    if (r == -2) return defer(fn, args, nargs);
    return PyBool_FromLong(r);
}

PyObject* py_condition_is(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 3) return defer(F_CONDITION_IS, args, nargs);
    return condition_is(F_CONDITION_IS, args, nargs, args[2], true);
}

PyObject* py_condition_is_true(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 2) return defer(F_CONDITION_IS_TRUE, args, nargs);
    return condition_is(F_CONDITION_IS_TRUE, args, nargs, S.True_, true);
}

PyObject* py_node_is_ready(PyObject*, PyObject* node) {
    return condition_is(F_NODE_IS_READY, &node, 1, S.True_, false);
}

// ---------------------------------------------------------------------------
// time
// ---------------------------------------------------------------------------

inline bool is_utc_datetime(PyObject* t) {
    if (!PyDateTime_CheckExact(t)) return false;
    PyDateTime_DateTime* dt = (PyDateTime_DateTime*)t;
    return dt->hastzinfo && dt->tzinfo == PyDateTime_TimeZone_UTC;
}

PyObject* rfc3339(int y, int mo, int d, int h, int mi, int s, int us) {
    char buf[48];
    int n = us < 0
        ? snprintf(buf, sizeof buf, "%04d-%02d-%02dT%02d:%02d:%02dZ", y, mo, d, h, mi, s)
        : snprintf(buf, sizeof buf, "%04d-%02d-%02dT%02d:%02d:%02d.%06dZ", y, mo, d, h, mi, s, us);
    return PyUnicode_FromStringAndSize(buf, n);
}

PyObject* fmt_datetime(PyObject* t, bool micro) {
    return rfc3339(PyDateTime_GET_YEAR(t), PyDateTime_GET_MONTH(t), PyDateTime_GET_DAY(t),
                   PyDateTime_DATE_GET_HOUR(t), PyDateTime_DATE_GET_MINUTE(t),
                   PyDateTime_DATE_GET_SECOND(t), micro ? PyDateTime_DATE_GET_MICROSECOND(t) : -1);
}

PyObject* py_fmt_time(PyObject*, PyObject* t) {
    if (!is_utc_datetime(t)) return defer(F_FMT_TIME, &t, 1);
    return fmt_datetime(t, false);
}

PyObject* py_fmt_micro_time(PyObject*, PyObject* t) {
    if (!is_utc_datetime(t)) return defer(F_FMT_MICRO_TIME, &t, 1);
    return fmt_datetime(t, true);
}

// The RFC 3339 string changes once a second: keep the one for the current
// second of the realtime clock (the clock datetime.now() reads).
time_t clock_sec;
PyObject* clock_str;

PyObject* now_rfc3339() {
    struct timespec ts;
    if (clock_gettime(CLOCK_REALTIME, &ts) != 0) return PyErr_SetFromErrno(PyExc_OSError);
    if (clock_str == nullptr || ts.tv_sec != clock_sec) {
        struct tm tm;
        if (gmtime_r(&ts.tv_sec, &tm) == nullptr) return PyErr_SetFromErrno(PyExc_OSError);
        PyObject* s = rfc3339(tm.tm_year + 1900, tm.tm_mon + 1, tm.tm_mday, tm.tm_hour,
                              tm.tm_min, tm.tm_sec, -1);
        if (s == nullptr) return nullptr;
        Py_XSETREF(clock_str, s);
        clock_sec = ts.tv_sec;
    }
    Py_INCREF(clock_str);
    return clock_str;
}

PyObject* py_now_rfc3339(PyObject*, PyObject*) { return now_rfc3339(); }

// ---------------------------------------------------------------------------
// uuid4_str
// ---------------------------------------------------------------------------

PyObject* py_uuid4_str(PyObject*, PyObject*) {
    unsigned char b[16];
    size_t have = 0;
    while (have < sizeof b) {
        ssize_t n = getrandom(b + have, sizeof b - have, 0);
        if (n < 0) {
            if (errno == EINTR) continue;
            return PyErr_SetFromErrno(PyExc_OSError);
        }
        have += (size_t)n;
    }
    b[6] = (unsigned char)((b[6] & 0x0f) | 0x40);  // version 4
    b[8] = (unsigned char)((b[8] & 0x3f) | 0x80);  // RFC 4122 variant
    static const char hex[] = "0123456789abcdef";
    char out[36];
    int o = 0;
    for (int i = 0; i < 16; i++) {
        if (i == 4 || i == 6 || i == 8 || i == 10) out[o++] = '-';
        out[o++] = hex[b[i] >> 4];
        out[o++] = hex[b[i] & 15];
    }
    return PyUnicode_FromStringAndSize(out, sizeof out);
}

// ---------------------------------------------------------------------------
// set_condition
// ---------------------------------------------------------------------------

inline bool same_name(PyObject* a, PyObject* b) {
    return a == b || (PyUnicode_CheckExact(a) && PyUnicode_Compare(a, b) == 0);
}

// set_condition(obj, cond_type, status, reason="", message="", *, at=None).
// Every shape is checked before the first write, so a deferred call finds
// the object untouched.
PyObject* py_set_condition(PyObject*, PyObject* const* args, Py_ssize_t nargs, PyObject* kwnames) {
    PyObject *reason = S.empty, *message = S.empty, *at = Py_None;
    bool ok = nargs >= 3 && nargs <= 5;
    if (ok) {
        if (nargs > 3) reason = args[3];
        if (nargs > 4) message = args[4];
        Py_ssize_t nkw = kwnames != nullptr ? PyTuple_GET_SIZE(kwnames) : 0;
        for (Py_ssize_t i = 0; ok && i < nkw; i++) {
            PyObject* k = PyTuple_GET_ITEM(kwnames, i);
            if (same_name(k, S.reason) && nargs <= 3) reason = args[nargs + i];
            else if (same_name(k, S.message) && nargs <= 4) message = args[nargs + i];
            else if (same_name(k, S.at)) at = args[nargs + i];
            else ok = false;
        }
    }
    if (!ok) return defer(F_SET_CONDITION, args, nargs, kwnames);
    PyObject *obj = args[0], *cond_type = args[1], *status = args[2];
    ok = PyDict_CheckExact(obj) && PyUnicode_CheckExact(cond_type) && PyUnicode_CheckExact(status) &&
         PyUnicode_CheckExact(reason) && PyUnicode_CheckExact(message) &&
         (at == Py_None || is_utc_datetime(at));
    if (!ok) return defer(F_SET_CONDITION, args, nargs, kwnames);

    PyObject *st = nullptr, *conds = nullptr, *existing = nullptr, *meta = nullptr, *gen = nullptr;
    int r = section(obj, S.status, &st);
    if (r == 1) {
        r = look(st, S.conditions, &conds);
        if (r == 1 && !PyList_CheckExact(conds)) r = -2;
    }
    if (r >= 0) r = section(obj, S.metadata, &meta);
    if (r == 1) r = look(meta, S.generation, &gen);
    if (r >= 0 && conds != nullptr) r = find_condition(obj, cond_type, &existing);
    int s_eq = 0, r_eq = 0, m_eq = 0;
    if (r >= 0 && existing != nullptr) {
        PyObject* v;
        r = s_eq = status_is(existing, status);
        if (r >= 0 && (r = look(existing, S.reason, &v)) >= 0)
            r = r_eq = fast_eq(v != nullptr ? v : Py_None, reason);
        if (r >= 0 && (r = look(existing, S.message, &v)) >= 0)
            r = m_eq = fast_eq(v != nullptr ? v : Py_None, message);
    }
    if (r == -1) return nullptr;
    if (r == -2) return defer(F_SET_CONDITION, args, nargs, kwnames);
    if (gen == nullptr) gen = long_zero;

    PyObject* ts = at == Py_None ? now_rfc3339() : fmt_datetime(at, false);
    if (ts == nullptr) return nullptr;
    Py_INCREF(gen);
    PyObject* result = nullptr;
    bool fail = false;
    if (st == nullptr) {
        st = PyDict_New();
        fail = st == nullptr || PyDict_SetItem(obj, S.status, st) < 0;
        Py_XDECREF(st);  // obj holds it now
    }
    if (!fail && conds == nullptr) {
        conds = PyList_New(0);
        fail = conds == nullptr || PyDict_SetItem(st, S.conditions, conds) < 0;
        Py_XDECREF(conds);
    }
    if (fail) {
        // nothing more to do
    } else if (existing == nullptr) {
        PyObject* c = PyDict_New();
        bool reason_set = PyUnicode_GET_LENGTH(reason) > 0;
        if (c != nullptr && PyDict_SetItem(c, S.type, cond_type) == 0 &&
            PyDict_SetItem(c, S.status, status) == 0 &&
            PyDict_SetItem(c, S.reason, reason_set ? reason : status) == 0 &&
            PyDict_SetItem(c, S.message, message) == 0 &&
            PyDict_SetItem(c, S.lastTransitionTime, ts) == 0 &&
            PyDict_SetItem(c, S.observedGeneration, gen) == 0 && PyList_Append(conds, c) == 0) {
            result = Py_True;
        }
        Py_XDECREF(c);
    } else {
        bool changed = false;
        Py_INCREF(existing);
        if (!s_eq) {
            fail = PyDict_SetItem(existing, S.status, status) < 0 ||
                   PyDict_SetItem(existing, S.lastTransitionTime, ts) < 0;
            changed = true;
        }
        if (!fail && PyUnicode_GET_LENGTH(reason) > 0 && !r_eq) {
            fail = PyDict_SetItem(existing, S.reason, reason) < 0;
            changed = true;
        }
        if (!fail && !m_eq) {
            fail = PyDict_SetItem(existing, S.message, message) < 0;
            changed = true;
        }
        if (!fail) fail = PyDict_SetItem(existing, S.observedGeneration, gen) < 0;
        Py_DECREF(existing);
        if (!fail) result = changed ? Py_True : Py_False;
    }
    Py_DECREF(gen);
    Py_DECREF(ts);
    Py_XINCREF(result);
    return result;
}

// ---------------------------------------------------------------------------
// Quantity: exact arithmetic on (numerator, denominator)
// ---------------------------------------------------------------------------
//
// The fast paths work in 64-bit values with 128-bit intermediates and answer
// None for anything wider or anything the grammar below does not cover; the
// caller then takes the Fraction route, so there is no overflow case.

typedef unsigned __int128 u128;
typedef __int128 i128;

const struct Suffix { const char* text; uint64_t num; uint64_t den; } suffixes[] = {
    {"", 1, 1}, {"m", 1, 1000},
    {"k", 1000ULL, 1}, {"M", 1000000ULL, 1}, {"G", 1000000000ULL, 1},
    {"T", 1000000000000ULL, 1}, {"P", 1000000000000000ULL, 1}, {"E", 1000000000000000000ULL, 1},
    {"Ki", 1ULL << 10, 1}, {"Mi", 1ULL << 20, 1}, {"Gi", 1ULL << 30, 1},
    {"Ti", 1ULL << 40, 1}, {"Pi", 1ULL << 50, 1}, {"Ei", 1ULL << 60, 1},
};

u128 gcd128(u128 a, u128 b) {
    while (b != 0) {
        u128 t = a % b;
        a = b;
        b = t;
    }
    return a;
}

inline bool is_digit(char c) { return c >= '0' && c <= '9'; }

// qty_parse(s) -> (num, den) in lowest terms, or None.
// Grammar: [+-]? (digits | digits? "." digits) letters*, at most 18 digits.
PyObject* py_qty_parse(PyObject*, PyObject* s) {
    if (!PyUnicode_CheckExact(s)) Py_RETURN_NONE;
    Py_ssize_t n;
    const char* p = PyUnicode_AsUTF8AndSize(s, &n);
    if (p == nullptr) return nullptr;
    Py_ssize_t i = 0;
    bool neg = false;
    if (i < n && (p[i] == '+' || p[i] == '-')) neg = p[i++] == '-';
    uint64_t mant = 0;
    int digits = 0, frac = 0;
    for (; i < n && is_digit(p[i]); i++) {
        if (++digits > 18) Py_RETURN_NONE;
        mant = mant * 10 + (uint64_t)(p[i] - '0');
    }
    if (i < n && p[i] == '.') {
        for (i++; i < n && is_digit(p[i]); i++, frac++) {
            if (++digits > 18) Py_RETURN_NONE;
            mant = mant * 10 + (uint64_t)(p[i] - '0');
        }
        if (frac == 0) Py_RETURN_NONE;
    }
    if (digits == 0) Py_RETURN_NONE;
    const Suffix* suf = nullptr;
    for (const Suffix& c : suffixes) {
        if ((Py_ssize_t)strlen(c.text) == n - i && memcmp(c.text, p + i, (size_t)(n - i)) == 0) {
            suf = &c;
            break;
        }
    }
    if (suf == nullptr) Py_RETURN_NONE;
    u128 num = (u128)mant * suf->num;  // < 2^60 * 2^61
    u128 den = suf->den;
    for (int k = 0; k < frac; k++) den *= 10;  // <= 10^21
    if (den != 1) {
        u128 g = gcd128(num, den);
        num /= g;
        den /= g;
    }
    if (num > (u128)INT64_MAX || den > (u128)INT64_MAX) Py_RETURN_NONE;
    long long sn = neg ? -(long long)num : (long long)num;
    return Py_BuildValue("(LL)", sn, (long long)den);
}

// _fmt_num on (num, den): integer, else whole milli-units, else str(float)
PyObject* fmt_ratio(PyObject* num, PyObject* den) {
    int overflow = 0;
    long long d = PyLong_AsLongLongAndOverflow(den, &overflow);
    if (d == -1 && !overflow && PyErr_Occurred()) return nullptr;
    if (!overflow && d == 1) return PyObject_Str(num);
    PyObject* milli = PyNumber_Multiply(num, long_thousand);
    if (milli == nullptr) return nullptr;
    PyObject* qr = PyNumber_Divmod(milli, den);
    Py_DECREF(milli);
    if (qr == nullptr) return nullptr;
    PyObject* out = nullptr;
    int rest = PyTuple_CheckExact(qr) && PyTuple_GET_SIZE(qr) == 2
        ? PyObject_IsTrue(PyTuple_GET_ITEM(qr, 1)) : -1;
    if (rest == 0) {
        out = PyUnicode_FromFormat("%Sm", PyTuple_GET_ITEM(qr, 0));
    } else if (rest > 0) {
        PyObject* f = PyNumber_TrueDivide(num, den);  // what float(Fraction) computes
        if (f != nullptr) out = PyObject_Str(f);
        Py_XDECREF(f);
    } else if (!PyErr_Occurred()) {
        PyErr_SetString(PyExc_TypeError, "qty_fmt(num, den) takes two ints");
    }
    Py_DECREF(qr);
    return out;
}

PyObject* py_qty_fmt(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 2 || !PyLong_Check(args[0]) || !PyLong_Check(args[1])) {
        PyErr_SetString(PyExc_TypeError, "qty_fmt(num, den) takes two ints");
        return nullptr;
    }
    return fmt_ratio(args[0], args[1]);
}

// qty_addsub(an, ad, bn, bd, subtract) -> (num, den, text) in lowest terms,
// or None when a value does not fit the 64-bit fast path
PyObject* py_qty_addsub(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 5) {
        PyErr_SetString(PyExc_TypeError, "qty_addsub(an, ad, bn, bd, subtract) takes 5 arguments");
        return nullptr;
    }
    long long v[4];
    for (int i = 0; i < 4; i++) {
        if (!PyLong_CheckExact(args[i])) Py_RETURN_NONE;
        int overflow = 0;
        v[i] = PyLong_AsLongLongAndOverflow(args[i], &overflow);
        if (overflow) Py_RETURN_NONE;
        if (v[i] == -1 && PyErr_Occurred()) return nullptr;
    }
    int sub = PyObject_IsTrue(args[4]);
    if (sub < 0) return nullptr;
    if (v[1] <= 0 || v[3] <= 0) Py_RETURN_NONE;
    i128 a = (i128)v[0] * v[3], b = (i128)v[2] * v[1];  // each below 2^126
    i128 num = sub ? a - b : a + b;
    u128 den = (u128)v[1] * (u128)v[3];
    bool neg = num < 0;
    u128 mag = neg ? (u128)(-num) : (u128)num;
    if (den != 1) {
        u128 g = gcd128(mag, den);
        mag /= g;
        den /= g;
    }
    if (mag > (u128)INT64_MAX || den > (u128)INT64_MAX) Py_RETURN_NONE;
    PyObject* pn = PyLong_FromLongLong(neg ? -(long long)mag : (long long)mag);
    PyObject* pd = PyLong_FromLongLong((long long)den);
    PyObject* text = (pn != nullptr && pd != nullptr) ? fmt_ratio(pn, pd) : nullptr;
    PyObject* out = text != nullptr ? PyTuple_Pack(3, pn, pd, text) : nullptr;
    Py_XDECREF(pn);
    Py_XDECREF(pd);
    Py_XDECREF(text);
    return out;
}

// ---------------------------------------------------------------------------
// field_index: the informer's fixed-path indexers
// ---------------------------------------------------------------------------

struct FieldIndex {
    PyObject_HEAD
    PyObject* py;     // the Python indexer for the same paths
    PyObject* paths;  // tuple of tuples of str
    vectorcallfunc vectorcall;
};

// None, or the list of non-empty strings at the paths, in path order. The
// top-level section is read as obj.get(k, {}), deeper maps as .get(k) or {}.
PyObject* field_index_values(FieldIndex* self, PyObject* obj) {
    PyObject* out = nullptr;
    bool plain = PyDict_CheckExact(obj);
    for (Py_ssize_t p = 0; plain && p < PyTuple_GET_SIZE(self->paths); p++) {
        PyObject* path = PyTuple_GET_ITEM(self->paths, p);
        Py_ssize_t n = PyTuple_GET_SIZE(path);
        PyObject* cur = obj;
        for (Py_ssize_t i = 0; cur != nullptr && plain && i < n - 1; i++) {
            PyObject* next;
            if (look(cur, PyTuple_GET_ITEM(path, i), &next) < 0) goto error;
            if (next == nullptr || (i > 0 && next == Py_None)) cur = nullptr;  // no value
            else if (PyDict_CheckExact(next)) cur = next;
            else plain = false;
        }
        if (cur == nullptr || !plain) continue;
        PyObject* v;
        if (look(cur, PyTuple_GET_ITEM(path, n - 1), &v) < 0) goto error;
        if (v == nullptr || v == Py_None) continue;
        if (!PyUnicode_CheckExact(v)) {
            plain = false;
        } else if (PyUnicode_GET_LENGTH(v) > 0) {
            if (out == nullptr && (out = PyList_New(0)) == nullptr) goto error;
            if (PyList_Append(out, v) < 0) goto error;
        }
    }
    if (!plain) {
        Py_XDECREF(out);
        return PyObject_CallOneArg(self->py, obj);
    }
    if (out == nullptr) Py_RETURN_NONE;
    return out;
error:
    Py_XDECREF(out);
    return nullptr;
}

PyObject* field_index_call(PyObject* self, PyObject* const* args, size_t nargsf, PyObject* kwnames) {
    FieldIndex* fi = (FieldIndex*)self;
    if (PyVectorcall_NARGS(nargsf) != 1 || (kwnames != nullptr && PyTuple_GET_SIZE(kwnames) > 0))
        return PyObject_Vectorcall(fi->py, args, nargsf, kwnames);
    return field_index_values(fi, args[0]);
}

void field_index_dealloc(PyObject* self) {
    FieldIndex* fi = (FieldIndex*)self;
    Py_XDECREF(fi->py);
    Py_XDECREF(fi->paths);
    Py_TYPE(self)->tp_free(self);
}

PyObject* field_index_repr(PyObject* self) {
    return PyUnicode_FromFormat("field_index%R", ((FieldIndex*)self)->paths);
}

PyTypeObject FieldIndexType = {PyVarObject_HEAD_INIT(nullptr, 0)};

bool ready_field_index_type() {
    FieldIndexType.tp_name = "_objmodel.FieldIndex";
    FieldIndexType.tp_basicsize = sizeof(FieldIndex);
    FieldIndexType.tp_dealloc = field_index_dealloc;
    FieldIndexType.tp_repr = field_index_repr;
    FieldIndexType.tp_call = PyVectorcall_Call;
    FieldIndexType.tp_vectorcall_offset = offsetof(FieldIndex, vectorcall);
    FieldIndexType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_VECTORCALL;
    FieldIndexType.tp_doc = "Indexer over fixed key paths; see kube/informer.py field_index.";
    return PyType_Ready(&FieldIndexType) == 0;
}

// field_index(py_indexer, *paths)
PyObject* py_field_index(PyObject*, PyObject* args) {
    Py_ssize_t n = PyTuple_GET_SIZE(args);
    if (n < 2 || !PyCallable_Check(PyTuple_GET_ITEM(args, 0))) {
        PyErr_SetString(PyExc_TypeError, "field_index(py_indexer, *paths) takes a callable and paths");
        return nullptr;
    }
    PyObject* paths = PyTuple_New(n - 1);
    if (paths == nullptr) return nullptr;
    for (Py_ssize_t i = 1; i < n; i++) {
        PyObject* path = PySequence_Tuple(PyTuple_GET_ITEM(args, i));
        if (path == nullptr) {
            Py_DECREF(paths);
            return nullptr;
        }
        PyTuple_SET_ITEM(paths, i - 1, path);
        bool ok = PyTuple_GET_SIZE(path) > 0;
        for (Py_ssize_t k = 0; ok && k < PyTuple_GET_SIZE(path); k++)
            ok = PyUnicode_CheckExact(PyTuple_GET_ITEM(path, k));
        if (!ok) {
            Py_DECREF(paths);
            PyErr_SetString(PyExc_TypeError, "a field_index path is a non-empty sequence of str");
            return nullptr;
        }
    }
    FieldIndex* fi = PyObject_New(FieldIndex, &FieldIndexType);
    if (fi == nullptr) {
        Py_DECREF(paths);
        return nullptr;
    }
    fi->py = PyTuple_GET_ITEM(args, 0);
    Py_INCREF(fi->py);
    fi->paths = paths;
    fi->vectorcall = field_index_call;
    return (PyObject*)fi;
}

// ---------------------------------------------------------------------------
// index_store: Informer._store / _reindex bookkeeping in one call
// ---------------------------------------------------------------------------

// fn(obj) normalised to None or a list (a str is one value)
PyObject* index_values(PyObject* fn, PyObject* obj) {
    if (obj == Py_None) Py_RETURN_NONE;
    PyObject* vals = Py_TYPE(fn) == &FieldIndexType ? field_index_values((FieldIndex*)fn, obj)
                                                    : PyObject_CallOneArg(fn, obj);
    if (vals == nullptr || vals == Py_None || PyList_CheckExact(vals)) return vals;
    PyObject* out = PyUnicode_Check(vals) ? PyList_New(0) : PySequence_List(vals);
    if (out != nullptr && PyUnicode_Check(vals) && PyList_Append(out, vals) < 0) Py_CLEAR(out);
    Py_DECREF(vals);
    return out;
}

// take `key` out of idx[v] for every v, dropping a bucket it empties: one
// empty set per value ever seen is an unbounded leak at churn rates
int buckets_remove(PyObject* idx, PyObject* vals, PyObject* key) {
    for (Py_ssize_t i = 0; i < PyList_GET_SIZE(vals); i++) {
        PyObject* v = PyList_GET_ITEM(vals, i);
        PyObject* s = PyDict_GetItemWithError(idx, v);
        if (s == nullptr) {
            if (PyErr_Occurred()) return -1;
            continue;
        }
        if (!PyAnySet_Check(s)) {
            PyErr_SetString(PyExc_TypeError, "an informer index bucket must be a set");
            return -1;
        }
        Py_INCREF(s);
        int rc = PySet_Discard(s, key);
        if (rc >= 0 && PySet_GET_SIZE(s) == 0) rc = PyDict_DelItem(idx, v);
        Py_DECREF(s);
        if (rc < 0) return -1;
    }
    return 0;
}

int buckets_add(PyObject* idx, PyObject* vals, PyObject* key) {
    for (Py_ssize_t i = 0; i < PyList_GET_SIZE(vals); i++) {
        PyObject* v = PyList_GET_ITEM(vals, i);
        PyObject* s = PyDict_GetItemWithError(idx, v);
        if (s == nullptr) {
            if (PyErr_Occurred()) return -1;
            s = PySet_New(nullptr);
            if (s == nullptr || PyDict_SetItem(idx, v, s) < 0) {
                Py_XDECREF(s);
                return -1;
            }
        } else {
            if (!PyAnySet_Check(s)) {
                PyErr_SetString(PyExc_TypeError, "an informer index bucket must be a set");
                return -1;
            }
            Py_INCREF(s);
        }
        int rc = PySet_Add(s, key);
        Py_DECREF(s);
        if (rc < 0) return -1;
    }
    return 0;
}

// index_store(key, old, new, indexes, cache): old/new are revisions or None.
// All index functions run first; buckets are touched only where the old and
// new values of an index differ; then cache[key] is set (or dropped).
PyObject* py_index_store(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 5 || !PyDict_Check(args[3]) || !PyDict_Check(args[4])) {
        PyErr_SetString(PyExc_TypeError,
                        "index_store(key, old, new, indexes, cache) takes 5 arguments, two dicts last");
        return nullptr;
    }
    PyObject *key = args[0], *old = args[1], *nw = args[2], *cache = args[4];
    PyObject* entries = PyDict_Values(args[3]);
    if (entries == nullptr) return nullptr;
    Py_ssize_t n = PyList_GET_SIZE(entries);
    PyObject* vals = PyTuple_New(2 * n);  // old values, new values per index
    bool ok = vals != nullptr;
    for (Py_ssize_t i = 0; ok && i < n; i++) {
        PyObject* e = PyList_GET_ITEM(entries, i);
        if (!PyTuple_CheckExact(e) || PyTuple_GET_SIZE(e) != 2 || !PyDict_Check(PyTuple_GET_ITEM(e, 1))) {
            PyErr_SetString(PyExc_TypeError, "an informer index is a (function, dict) pair");
            ok = false;
            break;
        }
        PyObject* ov = index_values(PyTuple_GET_ITEM(e, 0), old);
        if (ov == nullptr) { ok = false; break; }
        PyTuple_SET_ITEM(vals, 2 * i, ov);
        PyObject* nv = index_values(PyTuple_GET_ITEM(e, 0), nw);
        if (nv == nullptr) { ok = false; break; }
        PyTuple_SET_ITEM(vals, 2 * i + 1, nv);
    }
    for (Py_ssize_t i = 0; ok && i < n; i++) {
        PyObject* idx = PyTuple_GET_ITEM(PyList_GET_ITEM(entries, i), 1);
        PyObject* ov = PyTuple_GET_ITEM(vals, 2 * i);
        PyObject* nv = PyTuple_GET_ITEM(vals, 2 * i + 1);
        if (ov != Py_None && nv != Py_None) {
            int same = PyObject_RichCompareBool(ov, nv, Py_EQ);
            if (same < 0) ok = false;
            if (same != 0) continue;
        }
        if (ov != Py_None && buckets_remove(idx, ov, key) < 0) ok = false;
        if (ok && nv != Py_None && buckets_add(idx, nv, key) < 0) ok = false;
    }
    if (ok) {
        if (nw != Py_None) {
            ok = PyDict_SetItem(cache, key, nw) == 0;
        } else if (PyDict_DelItem(cache, key) < 0) {
            if (PyErr_ExceptionMatches(PyExc_KeyError)) PyErr_Clear();
            else ok = false;
        }
    }
    Py_XDECREF(vals);
    Py_DECREF(entries);
    if (!ok) return nullptr;
    Py_RETURN_NONE;
}

// ---------------------------------------------------------------------------
// module
// ---------------------------------------------------------------------------

#define FAST(f) (PyCFunction)(void (*)(void))f, METH_FASTCALL

PyMethodDef methods[] = {
    {"set_fallbacks", (PyCFunction)py_set_fallbacks, METH_O,
     "set_fallbacks(table): bind the Python bodies, by function name, that calls are "
     "handed to when the input is not a shape the fast path mirrors."},
    {"name_of", (PyCFunction)py_name_of, METH_O, "obj.get('metadata', {}).get('name', '')"},
    {"namespace_of", (PyCFunction)py_namespace_of, METH_O,
     "obj.get('metadata', {}).get('namespace', '')"},
    {"uid_of", (PyCFunction)py_uid_of, METH_O, "obj.get('metadata', {}).get('uid', '')"},
    {"labels_of", (PyCFunction)py_labels_of, METH_O, "obj.get('metadata', {}).get('labels') or {}"},
    {"annotations_of", (PyCFunction)py_annotations_of, METH_O,
     "obj.get('metadata', {}).get('annotations') or {}"},
    {"finalizers_of", (PyCFunction)py_finalizers_of, METH_O,
     "obj.get('metadata', {}).get('finalizers') or []"},
    {"owner_references_of", (PyCFunction)py_owner_references_of, METH_O,
     "obj.get('metadata', {}).get('ownerReferences') or []"},
    {"is_deleting", (PyCFunction)py_is_deleting, METH_O,
     "bool(obj.get('metadata', {}).get('deletionTimestamp'))"},
    {"provider_id_of", (PyCFunction)py_provider_id_of, METH_O,
     "node.get('spec', {}).get('providerID', '')"},
    {"has_finalizer", FAST(py_has_finalizer), "has_finalizer(obj, fin)"},
    {"object_key", (PyCFunction)py_object_key, METH_O, "'namespace/name', or 'name' when cluster-scoped"},
    {"get_condition", FAST(py_get_condition), "get_condition(obj, cond_type): the stored dict or None"},
    {"condition_is", FAST(py_condition_is), "condition_is(obj, cond_type, status)"},
    {"condition_is_true", FAST(py_condition_is_true), "condition_is_true(obj, cond_type)"},
    {"node_is_ready", (PyCFunction)py_node_is_ready, METH_O, "node_is_ready(node)"},
    {"node_ready_condition", (PyCFunction)py_node_ready_condition, METH_O,
     "node_ready_condition(node): the stored Ready condition or None"},
    {"set_condition", (PyCFunction)(void (*)(void))py_set_condition, METH_FASTCALL | METH_KEYWORDS,
     "set_condition(obj, cond_type, status, reason='', message='', *, at=None): True if changed"},
    {"fmt_time", (PyCFunction)py_fmt_time, METH_O, "RFC 3339 at second resolution"},
    {"fmt_micro_time", (PyCFunction)py_fmt_micro_time, METH_O, "RFC 3339 at microsecond resolution"},
    {"now_rfc3339", (PyCFunction)py_now_rfc3339, METH_NOARGS,
     "fmt_time(now()); the string of the current second is kept and returned again"},
    {"uuid4_str", (PyCFunction)py_uuid4_str, METH_NOARGS, "str(uuid.uuid4()) from the OS generator"},
    {"qty_parse", (PyCFunction)py_qty_parse, METH_O,
     "qty_parse(text) -> (num, den) in lowest terms, or None for the Fraction route"},
    {"qty_fmt", FAST(py_qty_fmt), "qty_fmt(num, den) -> text by the _fmt_num rules"},
    {"qty_addsub", FAST(py_qty_addsub),
     "qty_addsub(an, ad, bn, bd, subtract) -> (num, den, text), or None for the Fraction route"},
    {"field_index", (PyCFunction)py_field_index, METH_VARARGS,
     "field_index(py_indexer, *paths) -> indexer over fixed key paths"},
    {"index_store", FAST(py_index_store),
     "index_store(key, old, new, indexes, cache): update index buckets and the cache"},
    {nullptr, nullptr, 0, nullptr},
};

PyModuleDef moduledef = {
    PyModuleDef_HEAD_INIT, "_objmodel",
    "Native object-model core: accessors, conditions, timestamps, quantities, index store.", -1,
    methods, nullptr, nullptr, nullptr, nullptr,
};

bool intern_names() {
    struct { PyObject** slot; const char* text; } table[] = {
        {&S.metadata, "metadata"},
        {&S.name, "name"},
        {&S.namespace_, "namespace"},
        {&S.uid, "uid"},
        {&S.labels, "labels"},
        {&S.annotations, "annotations"},
        {&S.finalizers, "finalizers"},
        {&S.deletionTimestamp, "deletionTimestamp"},
        {&S.ownerReferences, "ownerReferences"},
        {&S.spec, "spec"},
        {&S.providerID, "providerID"},
        {&S.status, "status"},
        {&S.conditions, "conditions"},
        {&S.type, "type"},
        {&S.reason, "reason"},
        {&S.message, "message"},
        {&S.lastTransitionTime, "lastTransitionTime"},
        {&S.observedGeneration, "observedGeneration"},
        {&S.generation, "generation"},
        {&S.Ready, "Ready"},
        {&S.True_, "True"},
        {&S.empty, ""},
        {&S.at, "at"},
    };
    for (auto& e : table) {
        *e.slot = PyUnicode_InternFromString(e.text);
        if (*e.slot == nullptr) return false;
    }
    long_zero = PyLong_FromLong(0);
    long_thousand = PyLong_FromLong(1000);
    return long_zero != nullptr && long_thousand != nullptr;
}

}  // namespace

PyMODINIT_FUNC PyInit__objmodel(void) {
    PyDateTime_IMPORT;
    if (PyDateTimeAPI == nullptr) return nullptr;
    if (!intern_names() || !ready_field_index_type()) return nullptr;
    return PyModule_Create(&moduledef);
}
