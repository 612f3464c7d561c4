// _revstore: the success path of the in-memory apiserver's verbs
// (fake/apiserver.py), one native call per verb.
//
// Every claim passes through a few dozen writes, and what a write costs once
// the tree walks are native is interpreter glue: accessor calls, the rules of
// _apply_update, the resourceVersion counter, the history append and the scan
// over the watchers. The functions here run that glue against the server's
// own Python containers (the per-kind bucket of _store, _history, _watchers
// and the integer _rv), which keep their types and meaning:
//
//   get(bucket, namespace, name)
//   create(server, gvk, bucket, obj, validator, event_cap)
//   update(server, gvk, bucket, obj, subresource, validator)
//   patch(server, gvk, bucket, namespace, name, patch, subresource, validator)
//   delete(server, gvk, bucket, namespace, name, uid_precondition)
//   set_helpers(uuid4_str, now_rfc3339)
//
// A call either completes the write or touches nothing. Whatever would raise
// (not found, already exists, conflict, the finalizer rule, a validator
// violation, a uid precondition) and any input that is not plain wire format
// (a dict subclass, metadata that is not a dict, a key that is not a str)
// returns NotImplemented before the store, the counter, the history or a
// queue has been written; the caller then runs the Python body, which
// produces the exception and its message. Validation runs before the
// resourceVersion is issued, so a rejected write consumes none.
#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include <limits.h>

#include "jsontree_walk.h"

namespace {

using jsontree_walk::copy_tree;
using jsontree_walk::merge;
using jsontree_walk::merge_owned;

struct Names {
    PyObject *metadata, *name, *namespace_, *uid, *creationTimestamp, *generation,
        *deletionTimestamp, *finalizers, *resourceVersion, *spec, *status, *empty, *Event,
        *ADDED, *MODIFIED, *DELETED, *rv_attr, *history_attr, *watchers_attr, *append,
        *put_nowait;
} S;

PyObject* long_one;
PyObject* uuid4_str;    // bound with set_helpers
PyObject* now_rfc3339;  // bound with set_helpers

// an owned reference, dropped on scope exit
struct Ref {
    PyObject* p;
    explicit Ref(PyObject* o = nullptr) : p(o) {}
    ~Ref() { Py_XDECREF(p); }
    Ref(const Ref&) = delete;
    Ref& operator=(const Ref&) = delete;
    void reset(PyObject* o) { Py_XSETREF(p, o); }
    PyObject* release() {
        PyObject* o = p;
        p = nullptr;
        return o;
    }
    operator PyObject*() const { return p; }
};

inline PyObject* newref(PyObject* o) {
    Py_XINCREF(o);
    return o;
}

inline PyObject* miss() { Py_RETURN_NOTIMPLEMENTED; }

// d.get(key) on an exact dict: 1 found (*out borrowed), 0 absent, -1 error
inline int look(PyObject* d, PyObject* key, PyObject** out) {
    *out = PyDict_GetItemWithError(d, key);
    if (*out != nullptr) return 1;
    return PyErr_Occurred() ? -1 : 0;
}

// bool(d.get(key)): 1, 0, -1 error
inline int truthy(PyObject* d, PyObject* key) {
    PyObject* v;
    int r = look(d, key, &v);
    if (r <= 0) return r;
    Ref hold(newref(v));
    return PyObject_IsTrue(v);
}

inline bool str_eq(PyObject* a, PyObject* b) {
    return a == b || PyUnicode_Compare(a, b) == 0;
}

// (namespace or "", name) for plain strings; nullptr without an error set
// when either is something else
PyObject* make_key(PyObject* ns, PyObject* name) {
    if (ns == nullptr || ns == Py_None) ns = S.empty;
    if (name == nullptr || !PyUnicode_CheckExact(ns) || !PyUnicode_CheckExact(name)) return nullptr;
    return PyTuple_Pack(2, ns, name);
}

// the stored revision under `key` with its metadata: 1 found (both
// borrowed), 0 absent or not a plain revision, -1 error
int current(PyObject* bucket, PyObject* key, PyObject** cur, PyObject** cm) {
    int r = look(bucket, key, cur);
    if (r <= 0) return r;
    if (!PyDict_CheckExact(*cur)) return 0;
    r = look(*cur, S.metadata, cm);
    if (r == 1 && !PyDict_CheckExact(*cm)) return 0;
    return r;
}

// `if rv and rv != cur rv: conflict` for a requested resourceVersion found
// in `meta` (nullptr: no metadata): 1 passes, 0 conflict or odd shape, -1 error
int rv_precondition(PyObject* meta, PyObject* cm) {
    PyObject* want = nullptr;
    if (meta != nullptr && look(meta, S.resourceVersion, &want) < 0) return -1;
    if (want == nullptr || want == Py_None) return 1;
    if (!PyUnicode_CheckExact(want)) return 0;
    if (PyUnicode_GET_LENGTH(want) == 0) return 1;
    PyObject* have;
    int r = look(cm, S.resourceVersion, &have);
    if (r <= 0) return r;
    return PyUnicode_CheckExact(have) && str_eq(want, have);
}

// set(finalizers of new) - set(finalizers of cur) is empty: 1 yes, 0 no or
// odd shape, -1 error
int no_new_finalizers(PyObject* nm, PyObject* cm) {
    PyObject *nf, *cf;
    if (look(nm, S.finalizers, &nf) < 0 || look(cm, S.finalizers, &cf) < 0) return -1;
    if (nf == nullptr || nf == Py_None) return 1;
    if (cf == Py_None) cf = nullptr;
    if (!PyList_CheckExact(nf) || (cf != nullptr && !PyList_CheckExact(cf))) return 0;
    for (Py_ssize_t i = 0; i < PyList_GET_SIZE(nf); i++) {
        PyObject* f = PyList_GET_ITEM(nf, i);
        if (!PyUnicode_CheckExact(f)) return 0;
        bool found = false;
        for (Py_ssize_t j = 0; !found && cf != nullptr && j < PyList_GET_SIZE(cf); j++) {
            PyObject* c = PyList_GET_ITEM(cf, j);
            if (!PyUnicode_CheckExact(c)) return 0;
            found = str_eq(f, c);
        }
        if (!found) return 0;
    }
    return 1;
}

// validator(new, old) reports nothing: 1 valid, 0 violations, -1 error
int valid(PyObject* validator, PyObject* nw, PyObject* old) {
    if (validator == Py_None) return 1;
    PyObject* args[2] = {nw, old};
    Ref errs(PyObject_Vectorcall(validator, args, 2, nullptr));
    if (errs == nullptr) return -1;
    int t = PyObject_IsTrue(errs);
    return t < 0 ? -1 : !t;
}

// ---------------------------------------------------------------------------
// the commit: rv, store, history, watchers
// ---------------------------------------------------------------------------

// Where a write lands. Read in full before anything is written, so a server
// whose state is not the plain shape is left to the Python body untouched.
struct Sink {
    Ref append;    // _history.append, so a deque or a test's list both work
    Ref watchers;  // list of (gvk, queue)
    long long rv = 0;  // last issued
};

// 1 ready, 0 not the plain shape
int open_sink(PyObject* server, Sink& s) {
    Ref rv(PyObject_GetAttr(server, S.rv_attr));
    Ref hist(rv != nullptr ? PyObject_GetAttr(server, S.history_attr) : nullptr);
    if (hist != nullptr) s.append.reset(PyObject_GetAttr(hist, S.append));
    if (s.append != nullptr) s.watchers.reset(PyObject_GetAttr(server, S.watchers_attr));
    if (s.watchers == nullptr) {
        PyErr_Clear();  // the Python body meets the same and reports it
        return 0;
    }
    PyObject* ws = s.watchers.p;
    if (!PyLong_CheckExact(rv.p) || !PyList_CheckExact(ws)) return 0;
    int overflow = 0;
    s.rv = PyLong_AsLongLongAndOverflow(rv.p, &overflow);
    if (overflow || s.rv < 0 || s.rv == LLONG_MAX) return 0;
    for (Py_ssize_t i = 0; i < PyList_GET_SIZE(ws); i++) {
        PyObject* w = PyList_GET_ITEM(ws, i);
        if (!PyTuple_CheckExact(w) || PyTuple_GET_SIZE(w) != 2) return 0;
    }
    return 1;
}

// _bump + store (or remove) + the Event cap + _broadcast. `stored` is still
// private to this call and `nm` is its metadata. Everything that can fail for
// lack of memory is built before the first write. 0 done, -1 error.
int commit(PyObject* server, Sink& s, PyObject* gvk, PyObject* bucket, PyObject* key,
           PyObject* stored, PyObject* nm, PyObject* event_type, bool remove,
           Py_ssize_t cap = -1) {
    long long n = s.rv + 1;
    Ref rv_str(PyUnicode_FromFormat("%lld", n));
    Ref rv_int(PyLong_FromLongLong(n));
    if (rv_str == nullptr || rv_int == nullptr) return -1;
    Ref entry(PyTuple_Pack(4, (PyObject*)rv_int, gvk, event_type, stored));
    Ref event(PyTuple_Pack(2, event_type, stored));
    if (entry == nullptr || event == nullptr) return -1;
    if (PyDict_SetItem(nm, S.resourceVersion, rv_str) < 0) return -1;
    if (PyObject_SetAttr(server, S.rv_attr, rv_int) < 0) return -1;
    if ((remove ? PyDict_DelItem(bucket, key) : PyDict_SetItem(bucket, key, stored)) < 0) return -1;
    if (cap >= 0 && PyDict_GET_SIZE(bucket) > cap) {
        // oldest key first: dicts keep insertion order
        Py_ssize_t pos = 0;
        PyObject *k, *v;
        if (PyDict_Next(bucket, &pos, &k, &v)) {
            Ref oldest(newref(k));
            if (PyDict_DelItem(bucket, oldest) < 0) return -1;
        }
    }
    Ref appended(PyObject_CallOneArg(s.append, entry));
    if (appended == nullptr) return -1;
    PyObject* ws = s.watchers.p;
    for (Py_ssize_t i = 0; i < PyList_GET_SIZE(ws); i++) {
        PyObject* w = PyList_GET_ITEM(ws, i);
        if (!PyTuple_CheckExact(w) || PyTuple_GET_SIZE(w) != 2) continue;  // checked in open_sink
        Ref hold(newref(w));
        int eq = PyObject_RichCompareBool(PyTuple_GET_ITEM(w, 0), gvk, Py_EQ);
        if (eq < 0) return -1;
        if (!eq) continue;
        Ref put(PyObject_CallMethodOneArg(PyTuple_GET_ITEM(w, 1), S.put_nowait, event));
        if (put == nullptr) return -1;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// _apply_update
// ---------------------------------------------------------------------------

enum Mode {
    STATUS,        // obj is the caller's object: its status is copied
    STATUS_OWNED,  // obj is the merged status itself, already owned
    MAIN,          // obj is the caller's object: copied whole
    MAIN_OWNED,    // obj was built by the owned merge: taken as it is
};

// `cur` and its metadata `cm` are held by the caller for the whole call.
PyObject* apply_update(PyObject* server, PyObject* gvk, PyObject* bucket, PyObject* key,
                       PyObject* cur, PyObject* cm, PyObject* obj, Mode mode,
                       PyObject* validator) {
    Sink sink;
    if (!open_sink(server, sink)) return miss();
    Ref stored, meta_ref;
    bool remove = false;
    if (mode == STATUS || mode == STATUS_OWNED) {
        // a shallow re-root plus one status copy: everything else is shared
        // with the previous revision
        stored.reset(PyDict_Copy(cur));
        meta_ref.reset(PyDict_Copy(cm));
        if (stored == nullptr || meta_ref == nullptr) return nullptr;
        Ref status;
        if (mode == STATUS_OWNED) {
            status.reset(newref(obj));
        } else {
            PyObject* v;
            if (look(obj, S.status, &v) < 0) return nullptr;
            status.reset(v != nullptr ? copy_tree(v) : PyDict_New());
        }
        if (status == nullptr || PyDict_SetItem(stored, S.metadata, meta_ref) < 0 ||
            PyDict_SetItem(stored, S.status, status) < 0)
            return nullptr;
    } else {
        PyObject* om;
        int r = look(obj, S.metadata, &om);
        if (r < 0) return nullptr;
        if (r == 0 || !PyDict_CheckExact(om)) return miss();
        // once an object is terminating, new finalizers may not be added
        int deleting = truthy(cm, S.deletionTimestamp);
        if (deleting < 0) return nullptr;
        if (deleting) {
            r = no_new_finalizers(om, cm);
            if (r < 0) return nullptr;
            if (r == 0) return miss();
        }
        stored.reset(mode == MAIN_OWNED ? newref(obj) : copy_tree(obj));
        if (stored == nullptr) return nullptr;
        PyObject* v;
        // status is a subresource: a main-resource write keeps the stored one
        if (look(cur, S.status, &v) < 0) return nullptr;
        Ref status(v != nullptr ? newref(v) : PyDict_New());
        if (status == nullptr || PyDict_SetItem(stored, S.status, status) < 0) return nullptr;
        if (look(stored, S.metadata, &v) <= 0) return nullptr;
        meta_ref.reset(newref(v));
        // immutable metadata
        PyObject* fixed[4] = {S.uid, S.creationTimestamp, S.generation, S.deletionTimestamp};
        for (PyObject* f : fixed) {
            if (look(cm, f, &v) < 0) return nullptr;
            if (v != nullptr) {
                if (PyDict_SetItem(meta_ref, f, v) < 0) return nullptr;
            } else {
                int has = PyDict_Contains(meta_ref, f);
                if (has < 0 || (has && PyDict_DelItem(meta_ref, f) < 0)) return nullptr;
            }
        }
        PyObject *ns, *cs;
        if (look(stored, S.spec, &ns) < 0 || look(cur, S.spec, &cs) < 0) return nullptr;
        PyObject* a = ns != nullptr ? ns : Py_None;
        PyObject* b = cs != nullptr ? cs : Py_None;
        if (a != b) {  // else: shared with the previous revision, nothing to compare
            int ne = PyObject_RichCompareBool(a, b, Py_NE);
            if (ne < 0) return nullptr;
            if (ne) {
                PyObject* gen;
                if (look(cm, S.generation, &gen) < 0) return nullptr;
                if (gen == nullptr) gen = long_one;
                if (!PyLong_CheckExact(gen)) return miss();
                Ref next(PyNumber_Add(gen, long_one));
                if (next == nullptr || PyDict_SetItem(meta_ref, S.generation, next) < 0) return nullptr;
            } else if (ns != nullptr && cs != nullptr) {
                // re-share the equal spec: identity is what lets the
                // validator's changed-only walk prune in O(1)
                if (PyDict_SetItem(stored, S.spec, cs) < 0) return nullptr;
            }
        }
    }
    int ok = valid(validator, stored, cur);
    if (ok < 0) return nullptr;
    if (!ok) return miss();
    if (mode == MAIN || mode == MAIN_OWNED) {
        // removing the last finalizer of a deleting object removes it
        int deleting = truthy(meta_ref, S.deletionTimestamp);
        int fins = deleting > 0 ? truthy(meta_ref, S.finalizers) : 0;
        if (deleting < 0 || fins < 0) return nullptr;
        remove = deleting && !fins;
    }
    if (commit(server, sink, gvk, bucket, key, stored, meta_ref, remove ? S.DELETED : S.MODIFIED,
               remove) < 0)
        return nullptr;
    return copy_tree(stored);
}

inline bool is_gvk(PyObject* gvk) { return PyTuple_CheckExact(gvk) && PyTuple_GET_SIZE(gvk) == 2; }

// "" -> MAIN, "status" -> STATUS, anything else -> -1 (left to Python)
inline int subresource_mode(PyObject* sub) {
    if (!PyUnicode_CheckExact(sub)) return -1;
    if (PyUnicode_GET_LENGTH(sub) == 0) return MAIN;
    return str_eq(sub, S.status) ? STATUS : -1;
}

// ---------------------------------------------------------------------------
// verbs
// ---------------------------------------------------------------------------

PyObject* py_get(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 3) {
        PyErr_SetString(PyExc_TypeError, "get(bucket, namespace, name) takes 3 arguments");
        return nullptr;
    }
    if (!PyDict_Check(args[0])) return miss();
    Ref key(make_key(args[1], args[2]));
    if (key == nullptr) return PyErr_Occurred() ? nullptr : miss();
    PyObject* obj;
    int r = look(args[0], key, &obj);
    if (r < 0) return nullptr;
    if (r == 0) return miss();
    return copy_tree(obj);
}

PyObject* py_create(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 6) {
        PyErr_SetString(PyExc_TypeError,
                        "create(server, gvk, bucket, obj, validator, event_cap) takes 6 arguments");
        return nullptr;
    }
    PyObject *server = args[0], *gvk = args[1], *bucket = args[2], *obj = args[3],
             *validator = args[4];
    Py_ssize_t cap = PyLong_AsSsize_t(args[5]);
    if (cap == -1 && PyErr_Occurred()) return nullptr;
    if (!is_gvk(gvk) || !PyDict_Check(bucket) || !PyDict_CheckExact(obj) || uuid4_str == nullptr)
        return miss();
    PyObject* om;
    int r = look(obj, S.metadata, &om);
    if (r < 0) return nullptr;
    if (r == 0 || !PyDict_CheckExact(om)) return miss();
    PyObject *name, *ns;
    if (look(om, S.name, &name) < 0 || look(om, S.namespace_, &ns) < 0) return nullptr;
    if (name == nullptr || !PyUnicode_CheckExact(name) || PyUnicode_GET_LENGTH(name) == 0)
        return miss();
    Ref key(make_key(ns, name));
    if (key == nullptr) return PyErr_Occurred() ? nullptr : miss();
    r = PyDict_Contains(bucket, key);
    if (r < 0) return nullptr;
    if (r) return miss();  // already exists
    Sink sink;
    if (!open_sink(server, sink)) return miss();

    Ref stored(copy_tree(obj));
    if (stored == nullptr) return nullptr;
    PyObject* m;
    if (look(stored, S.metadata, &m) <= 0) return nullptr;
    Ref meta_ref(newref(m));
    // m["uid"] = m.get("uid") or uuid4_str(); the same for creationTimestamp
    struct { PyObject* key; PyObject* make; } fill[2] = {
        {S.uid, uuid4_str}, {S.creationTimestamp, now_rfc3339}};
    for (auto& f : fill) {
        int has = truthy(meta_ref, f.key);
        if (has < 0) return nullptr;
        if (has) continue;
        Ref v(PyObject_CallNoArgs(f.make));
        if (v == nullptr || PyDict_SetItem(meta_ref, f.key, v) < 0) return nullptr;
    }
    if (PyDict_SetItem(meta_ref, S.generation, long_one) < 0) return nullptr;
    // CRD schema; applies defaults into the fresh copy
    int ok = valid(validator, stored, Py_None);
    if (ok < 0) return nullptr;
    if (!ok) return miss();
    // Events are capped like a real cluster's event TTL would bound them
    PyObject* kind = PyTuple_GET_ITEM(gvk, 1);
    bool capped = PyUnicode_CheckExact(kind) && str_eq(kind, S.Event);
    if (commit(server, sink, gvk, bucket, key, stored, meta_ref, S.ADDED, false,
               capped ? cap : -1) < 0)
        return nullptr;
    return copy_tree(stored);
}

PyObject* py_update(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 6) {
        PyErr_SetString(PyExc_TypeError,
                        "update(server, gvk, bucket, obj, subresource, validator) takes 6 arguments");
        return nullptr;
    }
    PyObject *server = args[0], *gvk = args[1], *bucket = args[2], *obj = args[3];
    int mode = subresource_mode(args[4]);
    if (mode < 0 || !is_gvk(gvk) || !PyDict_Check(bucket) || !PyDict_CheckExact(obj)) return miss();
    PyObject* om;
    int r = look(obj, S.metadata, &om);
    if (r < 0) return nullptr;
    if (r == 0 || !PyDict_CheckExact(om)) return miss();
    PyObject *name, *ns;
    if (look(om, S.name, &name) < 0 || look(om, S.namespace_, &ns) < 0) return nullptr;
    Ref key(make_key(ns, name));
    if (key == nullptr) return PyErr_Occurred() ? nullptr : miss();
    PyObject *cur, *cm;
    r = current(bucket, key, &cur, &cm);
    if (r < 0) return nullptr;
    if (r == 0) return miss();  // not found
    Ref hold_cur(newref(cur)), hold_cm(newref(cm));
    r = rv_precondition(om, cm);
    if (r < 0) return nullptr;
    if (r == 0) return miss();  // conflict
    return apply_update(server, gvk, bucket, key, cur, cm, obj, (Mode)mode, args[5]);
}

PyObject* py_patch(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 8) {
        PyErr_SetString(PyExc_TypeError,
                        "patch(server, gvk, bucket, namespace, name, patch, subresource, validator) "
                        "takes 8 arguments");
        return nullptr;
    }
    PyObject *server = args[0], *gvk = args[1], *bucket = args[2], *patch = args[5];
    int mode = subresource_mode(args[6]);
    if (mode < 0 || !is_gvk(gvk) || !PyDict_Check(bucket) || !PyDict_CheckExact(patch)) return miss();
    Ref key(make_key(args[3], args[4]));
    if (key == nullptr) return PyErr_Occurred() ? nullptr : miss();
    PyObject *cur, *cm;
    int r = current(bucket, key, &cur, &cm);
    if (r < 0) return nullptr;
    if (r == 0) return miss();  // not found
    Ref hold_cur(newref(cur)), hold_cm(newref(cm));
    // metadata.resourceVersion in a merge patch is an optimistic-lock
    // precondition; without it, merge wins unconditionally
    PyObject* pm;
    r = look(patch, S.metadata, &pm);
    if (r < 0) return nullptr;
    if (r == 1 && !PyDict_CheckExact(pm)) return miss();
    r = rv_precondition(pm, cm);
    if (r < 0) return nullptr;
    if (r == 0) return miss();  // conflict
    if (mode == STATUS) {
        // fused owned merge of the status subtree: what the patch brings is
        // copied on the way in, the rest is shared with the current status,
        // and the result is stored as it is
        PyObject *sp, *cs;
        if (look(patch, S.status, &sp) < 0 || look(cur, S.status, &cs) < 0) return nullptr;
        Ref merged(merge(cs, sp != nullptr ? sp : patch, true));
        if (merged == nullptr) return nullptr;
        return apply_update(server, gvk, bucket, key, cur, cm, merged, STATUS_OWNED, args[7]);
    }
    PyObject* rv;
    r = look(cm, S.resourceVersion, &rv);
    if (r < 0) return nullptr;
    if (r == 0) return miss();
    Ref merged(merge_owned(cur, patch, S.metadata));
    if (merged == nullptr) return nullptr;
    PyObject* mm;
    r = PyDict_CheckExact(merged.p) ? look(merged, S.metadata, &mm) : 0;
    if (r < 0) return nullptr;
    if (r == 0 || !PyDict_CheckExact(mm)) return miss();
    if (PyDict_SetItem(mm, S.resourceVersion, rv) < 0) return nullptr;
    return apply_update(server, gvk, bucket, key, cur, cm, merged, MAIN_OWNED, args[7]);
}

// three outcomes: mark deleting, already deleting, remove
PyObject* py_delete(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 6) {
        PyErr_SetString(PyExc_TypeError,
                        "delete(server, gvk, bucket, namespace, name, uid_precondition) takes 6 arguments");
        return nullptr;
    }
    PyObject *server = args[0], *gvk = args[1], *bucket = args[2], *want_uid = args[5];
    if (!is_gvk(gvk) || !PyDict_Check(bucket) || !PyUnicode_CheckExact(want_uid) ||
        now_rfc3339 == nullptr)
        return miss();
    Ref key(make_key(args[3], args[4]));
    if (key == nullptr) return PyErr_Occurred() ? nullptr : miss();
    PyObject *cur, *cm;
    int r = current(bucket, key, &cur, &cm);
    if (r < 0) return nullptr;
    if (r == 0) return miss();  // not found
    Ref hold_cur(newref(cur)), hold_cm(newref(cm));
    if (PyUnicode_GET_LENGTH(want_uid) > 0) {
        PyObject* uid;
        if (look(cm, S.uid, &uid) < 0) return nullptr;
        if (uid == nullptr) uid = S.empty;
        if (!PyUnicode_CheckExact(uid) || !str_eq(uid, want_uid)) return miss();
    }
    int fins = truthy(cm, S.finalizers);
    int deleting = fins > 0 ? truthy(cm, S.deletionTimestamp) : 0;
    if (fins < 0 || deleting < 0) return nullptr;
    if (fins && deleting) Py_RETURN_NONE;
    Sink sink;
    if (!open_sink(server, sink)) return miss();
    Ref stored(PyDict_Copy(cur)), nm(PyDict_Copy(cm));
    Ref now(PyObject_CallNoArgs(now_rfc3339));
    if (stored == nullptr || nm == nullptr || now == nullptr ||
        PyDict_SetItem(stored, S.metadata, nm) < 0 ||
        PyDict_SetItem(nm, S.deletionTimestamp, now) < 0)
        return nullptr;
    if (commit(server, sink, gvk, bucket, key, stored, nm, fins ? S.MODIFIED : S.DELETED, !fins) < 0)
        return nullptr;
    Py_RETURN_NONE;
}

PyObject* py_set_helpers(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 2 || !PyCallable_Check(args[0]) || !PyCallable_Check(args[1])) {
        PyErr_SetString(PyExc_TypeError, "set_helpers(uuid4_str, now_rfc3339) takes two callables");
        return nullptr;
    }
    Py_XSETREF(uuid4_str, newref(args[0]));
    Py_XSETREF(now_rfc3339, newref(args[1]));
    Py_RETURN_NONE;
}

#define FAST(f) (PyCFunction)(void (*)(void))f, METH_FASTCALL

PyMethodDef methods[] = {
    {"set_helpers", FAST(py_set_helpers),
     "set_helpers(uuid4_str, now_rfc3339): bind the uid and clock functions create and delete call."},
    {"get", FAST(py_get), "get(bucket, namespace, name): a copy of the stored revision."},
    {"create", FAST(py_create),
     "create(server, gvk, bucket, obj, validator, event_cap): store a new object, return a copy."},
    {"update", FAST(py_update),
     "update(server, gvk, bucket, obj, subresource, validator): replace the main resource or the "
     "status, return a copy."},
    {"patch", FAST(py_patch),
     "patch(server, gvk, bucket, namespace, name, patch, subresource, validator): merge patch the "
     "main resource or the status, return a copy."},
    {"delete", FAST(py_delete),
     "delete(server, gvk, bucket, namespace, name, uid_precondition): mark deleting or remove."},
    {nullptr, nullptr, 0, nullptr},
};

PyModuleDef moduledef = {
    PyModuleDef_HEAD_INIT, "_revstore",
    "Native success path of the in-memory apiserver's verbs; every entry point returns "
    "NotImplemented, with nothing touched, for what the Python body has to handle.",
    -1, methods, nullptr, nullptr, nullptr, nullptr,
};

bool intern_names() {
    struct { PyObject** slot; const char* text; } table[] = {
        {&S.metadata, "metadata"},
        {&S.name, "name"},
        {&S.namespace_, "namespace"},
        {&S.uid, "uid"},
        {&S.creationTimestamp, "creationTimestamp"},
        {&S.generation, "generation"},
        {&S.deletionTimestamp, "deletionTimestamp"},
        {&S.finalizers, "finalizers"},
        {&S.resourceVersion, "resourceVersion"},
        {&S.spec, "spec"},
        {&S.status, "status"},
        {&S.empty, ""},
        {&S.Event, "Event"},
        {&S.ADDED, "ADDED"},
        {&S.MODIFIED, "MODIFIED"},
        {&S.DELETED, "DELETED"},
        {&S.rv_attr, "_rv"},
        {&S.history_attr, "_history"},
        {&S.watchers_attr, "_watchers"},
        {&S.append, "append"},
        {&S.put_nowait, "put_nowait"},
    };
    for (auto& e : table) {
        *e.slot = PyUnicode_InternFromString(e.text);
        if (*e.slot == nullptr) return false;
    }
    long_one = PyLong_FromLong(1);
    return long_one != nullptr;
}

}  // namespace

PyMODINIT_FUNC PyInit__revstore(void) {
    if (!intern_names()) return nullptr;
    return PyModule_Create(&moduledef);
}
