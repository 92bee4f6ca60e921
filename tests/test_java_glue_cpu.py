"""The reference-side Java glue (java/) cannot be compiled here -- no JDK in the image.  What can be checked is checked:
* tools/check_java_glue.py (run by hand with --reference <the reference's checkout>: every reference class / member /
  constructor the glue uses exists in the reference's sources with that name, arity and a visibility the glue can reach)
  flags the mistakes it is meant to catch and nothing else: a deliberately broken class and a correct one, both against a
  small library of the test's own standing in for the reference;
* java/jni/gsgpu_jni.c passes `gcc -fsyntax-only` against a declarations-only jni.h and implements exactly the native
  methods GsGpuNative.java declares, with matching argument counts, calling only functions include/gsgpu.h declares."""
import os
import re
import subprocess
import sys

from conftest import ROOT

CHECK = os.path.join(ROOT, "tools", "check_java_glue.py")

# the stand-in library: laid out as the checker looks for sources (core|base/src/main/java), one of each kind of
# declaration the checks below need -- constructors of one arity, a final and an overridable hook, a private field, nested
# classes, an interface method, enum constants
LIBRARY = {
    "core/src/main/java/org/example/lib/Matcher.java": '''
package org.example.lib;

import java.io.IOException;
import org.example.lib.store.Store;

public class Matcher {
	protected final Store store;
	private Object callback;

	public Matcher(Store store, int threads, Context context) {
		this.store = store;
	}

	protected final void nextEntry(Entry entry, int index) throws IOException {
	}

	protected boolean matchRead(Entry entry, int index) {
		return false;
	}

	public static class Entry {
		public void growBuffer(int n) {
		}
	}

	public static class Counts {
		public long reads;
	}
}
''',
    "core/src/main/java/org/example/lib/Context.java": '''
package org.example.lib;

public class Context {
	public Context(int threads) {
	}
}
''',
    "base/src/main/java/org/example/lib/store/Store.java": '''
package org.example.lib.store;

public interface Store {
	long getValues(int index);
}
''',
    "base/src/main/java/org/example/lib/Key.java": '''
package org.example.lib;

public enum Key {
	THREADS, LOG_LEVEL;
}
''',
}

BROKEN = '''
package org.example.lib;

import java.io.IOException;
import org.example.lib.Key;
import org.example.lib.store.Store;

public class Broken extends Matcher {
	public Broken(Store store, Context context) {
		super(store, 1, 2, context);                             // no such constructor arity
	}

	@Override
	protected void nextEntry(Entry entry, int index) throws IOException {   // final in Matcher
	}

	@Override
	protected void noSuchHook(int x) {                           // nothing to override
	}

	void use(Counts stats, Entry e) {
		stats.noSuchField = 1;                                   // unknown member
		Object o = callback;                                     // private field of the superclass
		long n = store.getValues(1, 2);                          // wrong arity
		Object key = Key.NO_SUCH_KEY;                            // unknown constant
		e.growBufferTypo(3);                                     // unknown method on a library type
		Matcher m = new Matcher(store) {                         // constructor arity + bogus override in an anonymous class
			@Override
			protected boolean matchReadTypo(Entry entry, int index) {
				return false;
			}
		};
	}
}
'''

GOOD = '''
package org.example.glue;

import org.example.lib.Context;
import org.example.lib.Key;
import org.example.lib.Matcher;
import org.example.lib.store.Store;

public class Good extends Matcher {
	private final Context own;

	public Good(Store store, Context context) {
		super(store, 2, context);
		own = new Context(2);
	}

	@Override
	protected boolean matchRead(Entry entry, int index) {
		entry.growBuffer(index);
		return store.getValues(index) > 0 && Key.THREADS != null;
	}

	long count(Counts stats) {
		Matcher m = new Matcher(store, 1, own) {
			@Override
			protected boolean matchRead(Entry entry, int index) {
				return true;
			}
		};
		return stats.reads;
	}
}
'''


def test_checker_flags_what_it_is_meant_to_catch(tmp_path):
    ref = tmp_path / "ref"
    for rel, text in LIBRARY.items():
        (ref / rel).parent.mkdir(parents=True, exist_ok=True)
        (ref / rel).write_text(text)
    glue = tmp_path / "glue"
    for pkg, name, text in (("lib", "Broken", BROKEN), ("glue", "Good", GOOD)):
        d = glue / "org" / "example" / pkg
        d.mkdir(parents=True)
        (d / (name + ".java")).write_text(text)
    r = subprocess.run([sys.executable, CHECK, "--reference", str(ref), "--glue", str(glue)], capture_output=True, text=True)
    assert r.returncode == 1
    out = r.stdout
    assert re.search(r"checked 2 glue classes against %d reference files" % len(LIBRARY), out), out
    for needle in ("super(...) with 4 arguments", "@Override nextEntry", "is final", "@Override noSuchHook", "noSuchField",
                   "callback is private", "getValues(...): no overload takes 2", "NO_SUCH_KEY",
                   "growBufferTypo", "new Matcher(...) with 1 arguments", "@Override matchReadTypo"):
        assert needle in out, (needle, out)
    assert "Good" not in out, out


def test_jni_shim_syntax_and_coverage():
    src = os.path.join(ROOT, "java", "jni", "gsgpu_jni.c")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror", "-fsyntax-only",
                        "-I" + os.path.join(ROOT, "tests", "native", "jni_stub"), "-I" + os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    java = open(os.path.join(ROOT, "java", "src", "org", "metagene", "genestrip", "gpu", "GsGpuNative.java")).read()
    natives = {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
               for m in re.finditer(r"static\s+native\s+[\w\[\]]+\s+(\w+)\s*\(([^)]*)\)", java, re.S)}
    c = open(src).read()
    impl = {m.group(1): len([a for a in m.group(2).split(",") if a.strip()]) - 2  # JNIEnv *, jclass
            for m in re.finditer(r"JNAME\((\w+)\)\s*\(([^)]*)\)", c, re.S)}
    assert natives == impl, (set(natives) ^ set(impl), {k: (natives[k], impl[k]) for k in natives if k in impl and natives[k] != impl[k]})
    assert len(natives) >= 26
    header = open(os.path.join(ROOT, "include", "gsgpu.h")).read() + open(os.path.join(ROOT, "include", "gshost.h")).read()
    declared = set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", header))
    called = set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", c))
    assert called <= declared, called - declared
    # the file-level flows of the reference's seam (runMatcher / runFilter over local files) are bound (missing 2)
    for name in ("hostMatchFiles", "hostMatchRun", "hostMatchInto", "hostFilterFiles", "hostLastError"):
        assert name in natives, name
    glue = open(os.path.join(ROOT, "java", "src", "org", "metagene", "genestrip", "match", "GpuFastqKMerMatcher.java")).read()
    assert "GsGpuNative.hostMatchRun(" in glue and "GsGpuNative.matchSubmitAsync(" in glue and "GsGpuNative.matchSubmit(" not in glue
    glue = open(os.path.join(ROOT, "java", "src", "org", "metagene", "genestrip", "bloom", "GpuFastqBloomFilter.java")).read()
    assert "GsGpuNative.hostFilterFiles(" in glue
